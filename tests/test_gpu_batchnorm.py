"""The BatchNorm (+ LeakyReLU) kernels of csrc/batchnorm.hip against their formulas in fp64 (torch on the CPU), through ops.bn_* and
autograd.batch_norm_act, and the dtype refusal / empty problem of every new entry point through the C ABI.

Shapes: spatial (6, 10), (7, 7), (3, 2, 5) and one of 4 100 rows (more than one row block of every pass); N in 1 .. 3; C in 1, 3, 8, 12, 40, 64 (the
vector form, the scalar form, and C = 12: vector in fp32, scalar in bf16); dense operands and channel slices of wider buffers (pitch != C: nothing
outside the slice may change); slope 0, 0.2 and no activation; train and eval.  Bars: the project's kernel bars -- 1e-4 * max(1, |ref|max) in fp32, 2e-2 of
that scale in bf16 (both sides start from the same bf16-representable operands; the reference is fp64)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from generativemodels_amd import _native as nat
from generativemodels_amd import autograd as A
from generativemodels_amd import ops

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
BAR = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
# (N, spatial, C, slope, sliced)
SHAPES = [
    (2, (6, 10), 8, 0.2, False),
    (1, (7, 7), 3, 0.0, False),
    (3, (3, 2, 5), 12, None, False),
    (2, (7, 7), 1, 0.2, False),
    (2, (6, 10), 40, 0.2, True),
    (3, (7, 7), 64, 0.0, True),
    (1, (3, 2, 5), 3, None, True),
    (2, (50, 41), 8, 0.2, False),  # 4 100 rows: several row blocks in every pass
    (1, (4100,), 12, 0.2, True),
]
IDS = [f"N{n}-{'x'.join(map(str, sp))}-C{c}-slope{s}-{'slice' if sl else 'dense'}" for n, sp, c, s, sl in SHAPES]


def _close(got, want, bar, what):
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = bar * max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item() if want.numel() else 0.0
    print(f"{what}: max|err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e}"


def _operands(n, sp, c, dtype, sliced, seed):
    """x, gy as arena tensors (slices of wider buffers filled with a sentinel when `sliced`), and gamma, beta, running buffers on the CPU in fp32."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, *sp, c)
    x = (torch.randn(shape, generator=g) * 1.5 + 0.5).to(dtype)
    gy = torch.randn(shape, generator=g).to(dtype)
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    beta = 0.2 * torch.randn(c, generator=g)
    rm = 0.1 * torch.randn(c, generator=g)
    rv = 0.5 + torch.rand(c, generator=g)

    def place(t):
        if not sliced:
            return t.cuda(), None
        wide = torch.full((n, *sp, c + 8), 77.0, dtype=dtype, device="cuda")
        view = wide[..., 4:4 + c] if c % 4 else wide[..., 8:]  # (an unaligned slice for the scalar form, an aligned one for the vector form)
        view.copy_(t)
        return view, wide
    return x, gy, place, gamma, beta, rm, rv


def _reference(x, gy, gamma, beta, rm, rv, training, slope):
    """fp64 autograd of F.batch_norm + leaky_relu over channels-last operands -> y, dx, dgamma, dbeta, running buffers after the call."""
    xr = x.double().movedim(-1, 1).clone().requires_grad_(True)
    ga, be = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xr, rm64, rv64, ga, be, training, MOMENTUM, EPS)
    if slope is not None:
        y = F.leaky_relu(y, slope)
    y.backward(gy.double().movedim(-1, 1))
    return y.detach().movedim(1, -1), xr.grad.movedim(1, -1), ga.grad, be.grad, rm64, rv64


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,sp,c,slope,sliced", SHAPES, ids=IDS)
def test_forward_backward_and_running_buffers(n, sp, c, slope, sliced, dtype, training):
    x, gy, place, gamma, beta, rm, rv = _operands(n, sp, c, dtype, sliced, 1000 + c + n)
    y_ref, dx_ref, dg_ref, db_ref, rm_ref, rv_ref = _reference(x, gy, gamma, beta, rm, rv, training, slope)
    xd, xwide = place(x)
    gd, _ = place(gy)
    rows = ops.rows_of(xd)
    gam, bet, rmd, rvd = gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()
    stats = ops.channel_stats(xd) if training else None
    scale, shift, mean, invstd = ops.bn_finalize(stats, rows, c, gam, bet, rmd, rvd, training, MOMENTUM, EPS)
    out = wide_out = None
    if sliced:
        wide_out = torch.full((n, *sp, c + 8), 77.0, dtype=dtype, device="cuda")
        out = wide_out[..., 4:4 + c] if c % 4 else wide_out[..., 8:]
    y = ops.bn_apply(xd, scale, shift, slope, out=out)
    dx, dgamma, dbeta = ops.bn_backward(xd, gd, scale, shift, mean, invstd, training, slope)
    bar = BAR[dtype]
    _close(y, y_ref, bar, "y")
    _close(dx, dx_ref, bar, "dx")
    _close(dgamma, dg_ref, bar, "dgamma")
    _close(dbeta, db_ref, bar, "dbeta")
    # the running buffers are fp32 whatever the storage dtype: torch's formula (unbiased variance, momentum), or untouched in eval
    _close(rmd, rm_ref, 1e-5, "running_mean")
    _close(rvd, rv_ref, 1e-5, "running_var")
    if not training:
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    if sliced:  # nothing outside the slices changed
        lo, hi = (4, 4 + c) if c % 4 else (8, 8 + c)
        for wide in (xwide, wide_out):
            keep = torch.ones(c + 8, dtype=torch.bool)
            keep[lo:hi] = False
            assert bool((wide[..., keep.cuda()] == 77.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_identical_calls_are_bitwise_equal(dtype):
    n, sp, c = 2, (50, 41), 40
    x, gy, place, gamma, beta, rm, rv = _operands(n, sp, c, dtype, False, 7)
    got = []
    for _ in range(2):
        xd, gd = x.cuda().requires_grad_(True), gy.cuda()
        gam, bet = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
        rmd, rvd = rm.cuda(), rv.cuda()
        y = A.batch_norm_act(xd, gam, bet, rmd, rvd, True, MOMENTUM, EPS, 0.2)
        y.backward(gd)
        got.append((y.detach(), xd.grad, gam.grad, bet.grad, rmd, rvd))
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_autograd_two_forwards_before_one_backward_and_no_grad_updates_buffers():
    """D(fake), D(real), one backward: each call's backward reads its own tables; the buffers see both updates; torch.no_grad() in training mode still updates."""
    n, sp, c = 2, (6, 10), 8
    xa, gya, _, gamma, beta, rm, rv = _operands(n, sp, c, torch.float32, False, 11)
    xb, gyb, *_ = _operands(n, sp, c, torch.float32, False, 12)
    xb = xb * 2.0 - 1.0
    # fp64 reference: two calls in order, one backward of the sum
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    xs = [t.double().movedim(-1, 1).clone().requires_grad_(True) for t in (xa, xb)]
    ys = [F.leaky_relu(F.batch_norm(t, rm64, rv64, ga, be, True, MOMENTUM, EPS), 0.2) for t in xs]
    (ys[0] * gya.double().movedim(-1, 1)).sum().add((ys[1] * gyb.double().movedim(-1, 1)).sum()).backward()
    gam, bet, rmd, rvd = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True), rm.cuda(), rv.cuda()
    xd = [t.cuda().requires_grad_(True) for t in (xa, xb)]
    yd = [A.batch_norm_act(t, gam, bet, rmd, rvd, True, MOMENTUM, EPS, 0.2) for t in xd]
    ((yd[0] * gya.cuda()).sum() + (yd[1] * gyb.cuda()).sum()).backward()
    for i in range(2):
        _close(xd[i].grad, xs[i].grad.movedim(1, -1), 1e-4, f"dx of call {i}")
    _close(gam.grad, ga.grad, 1e-4, "dgamma")
    _close(bet.grad, be.grad, 1e-4, "dbeta")
    _close(rmd, rm64, 1e-5, "running_mean after two calls")
    _close(rvd, rv64, 1e-5, "running_var after two calls")
    before = rmd.clone()
    with torch.no_grad():
        A.batch_norm_act(xd[0].detach(), gam, bet, rmd, rvd, True, MOMENTUM, EPS, 0.2)
    F.batch_norm(xs[0].detach(), rm64, rv64, None, None, True, MOMENTUM, EPS)
    assert not torch.equal(before, rmd)
    _close(rmd, rm64, 1e-5, "running_mean after a no_grad call")


def test_one_value_per_channel_is_refused_in_training():
    x = torch.randn(1, 1, 1, 8, device="cuda")
    rm, rv = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        A.batch_norm_act(x, None, None, rm, rv, True, MOMENTUM, EPS, 0.2)
    A.batch_norm_act(x, None, None, rm, rv, False, MOMENTUM, EPS, 0.2)  # eval normalises with the running buffers


def test_bf16_buffers_make_an_fp32_round_trip():
    n, sp, c = 2, (6, 10), 8
    x, _, _, gamma, beta, rm, rv = _operands(n, sp, c, torch.bfloat16, False, 5)
    _, _, _, _, rm_ref, rv_ref = _reference(x, torch.zeros_like(x), gamma.bfloat16().float(), beta.bfloat16().float(), rm.bfloat16().float(), rv.bfloat16().float(), True, 0.2)
    rmd, rvd = rm.bfloat16().cuda(), rv.bfloat16().cuda()
    A.batch_norm_act(x.cuda(), gamma.bfloat16().cuda(), beta.bfloat16().cuda(), rmd, rvd, True, MOMENTUM, EPS, 0.2)
    assert rmd.dtype == torch.bfloat16 and rvd.dtype == torch.bfloat16
    for got, want in ((rmd, rm_ref), (rvd, rv_ref)):  # one bf16 rounding of the fp32 result
        assert (got.cpu().double() - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item()


# ---- the dtype refusal and the empty problem, in the form of tests/test_gpu_dtype_refusal.py -----------------------------------------------------------
F32, F16, BAD = 0, 2, 7
SENTINEL = 123.0


class Ctx:
    def __init__(self):
        self.outs, self.keep = [], []
        self.s = torch.cuda.current_stream().cuda_stream

    def i(self, n=16):
        t = (torch.arange(n, dtype=torch.float32) / 8 - 0.75).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def o(self, n=16, dtype=torch.float32):
        t = torch.full((n,), SENTINEL, dtype=dtype, device="cuda")
        self.outs.append(t)
        return t.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outs)


# name -> (call(L, k, dtype, n), n of the 16-element problem, return value of the empty problem with a dtype that is not served)
SPECS = {
    "gm_bn_apply": (lambda L, k, d, n: L.gm_bn_apply(k.i(), 8, k.o(), 8, k.i(), k.i(), n, 8, 1, 0.2, d, k.s), 2, 0),
    "gm_bn_bwd_stats": (lambda L, k, d, n: L.gm_bn_bwd_stats(k.i(), 8, k.i(), 8, k.i(), k.i(), k.i(), k.i(), n, 8, 1, 0.2, k.o(16, torch.float64), d, k.s), 2, 0),
    "gm_bn_bwd_apply": (lambda L, k, d, n: L.gm_bn_bwd_apply(k.i(), 8, k.i(), 8, k.o(), 8, k.i(), k.i(), k.i(), k.i(), k.i(), n, 8, 1, 0.2, d, k.s), 2, 0),
    # (no elements: the loss is 0, and is written -- like gm_kld)
    "gm_patch_adv_loss": (lambda L, k, d, n: L.gm_patch_adv_loss(k.i(), n, 2, 1, 1.0, 1.0, k.o(), None, None, None, k.o(), d, k.s), 16, -2),
}


@pytest.mark.parametrize("d", [BAD, F16], ids=["unknown", "fp16"])
@pytest.mark.parametrize("name", sorted(SPECS))
def test_unserved_dtype_is_refused(name, d):
    L = nat.lib()
    call, n, _ = SPECS[name]
    assert L.gm_scale(None, None, 1.0, 0, 1, F32, None) == -1  # a different message into the error slot
    k = Ctx()
    rc = call(L, k, d, n)
    assert rc == -2, f"{name} with dtype {d}: returned {rc} ({L.gm_last_error()})"
    assert L.gm_last_error() == f"{name}: error -2: unsupported dtype".encode()
    assert k.untouched(), f"{name} with dtype {d}: an output changed"


@pytest.mark.parametrize("name", sorted(SPECS))
def test_empty_problem(name):
    L = nat.lib()
    call, _, want = SPECS[name]
    k = Ctx()
    rc = call(L, k, BAD, 0)
    assert rc == want, f"{name}, empty problem with dtype {BAD}: returned {rc}, expected {want} ({L.gm_last_error()})"
    assert k.untouched()
    k = Ctx()
    assert call(L, k, F32, 0) == 0, L.gm_last_error()  # a served dtype: nothing to do for the streaming passes, the value 0 for the loss
    torch.cuda.synchronize()
    if name == "gm_patch_adv_loss":
        assert float(k.outs[0][0]) == 0.0 and bool((k.outs[1] == SENTINEL).all())
    else:
        assert k.untouched()


def test_finalize_entry_points_take_no_dtype_and_check_their_arguments():
    """gm_bn_finalize / gm_bn_bwd_finalize read fp64 partials and fp32 tables only; no channels is the empty problem, missing operands are refused."""
    L = nat.lib()
    k = Ctx()
    assert L.gm_bn_finalize(None, 0, 0, 0, 0, None, None, 1e-5, 0.1, 0, k.i(), k.i(), k.o(), k.o(), None, None, k.s) == 0
    assert L.gm_bn_finalize(None, 1, 1, 8, 2, None, None, 1e-5, 0.1, 1, None, None, k.o(), k.o(), None, None, k.s) == -1  # training without partials
    assert L.gm_bn_finalize(None, 0, 0, 8, 0, None, None, 1e-5, 0.1, 0, None, None, k.o(), k.o(), None, None, k.s) == -1  # eval without running buffers
    assert L.gm_bn_bwd_finalize(k.i(), 1, 0, 2, k.i(), k.i(), 1, None, None, k.o(), k.o(), k.s) == 0
    assert L.gm_bn_bwd_finalize(None, 1, 8, 2, k.i(), k.i(), 1, None, None, k.o(), k.o(), k.s) == -1
    assert k.untouched()
    assert L.gm_bn_bwd_stats_slots(0) == 0 and L.gm_bn_bwd_stats_slots(256) == 1 and L.gm_bn_bwd_stats_slots(4100) > 1
    assert isinstance(C.c_longlong(L.gm_bn_bwd_stats_slots(1 << 40)).value, int) and L.gm_bn_bwd_stats_slots(1 << 40) <= 1024
