"""The dtype refusal of the streaming entry points (csrc: gm_dispatch_dtype / gm_dispatch_vec), pinned through the C ABI.

Every entry point of elementwise / groupnorm / backward (below the weight gradient) / spade_net / transformer_ops / vq / metrics / resize .hip that
takes a dtype is called with real 16-element device tensors and a dtype code it does not serve: it returns -2, gm_last_error() reads
"<its own name>: error -2: unsupported dtype", and no output changes.  Only the three metric entry points serve GM_F16.  An empty problem returns 0
before the dtype is looked at wherever the entry point has such an early return; the few that have none (or that reject an empty input) are pinned
too.  Arguments are valid for every other check, so -2 is the dtype's doing, and nothing is launched, so nothing can fault."""
import ctypes as C

import pytest
import torch

from generativemodels_amd import _native as nat

pytestmark = pytest.mark.gpu

F32, BF16, F16, BAD = 0, 1, 2, 7
SENTINEL = 123.0


class Ctx:
    """16-element device tensors: inputs i(), outputs o() (filled with a sentinel and checked by untouched()), int64 indices, the stream."""

    def __init__(self, in_dtype=torch.float32):
        self.in_dtype, self.outs, self.keep = in_dtype, [], []
        self.s = torch.cuda.current_stream().cuda_stream

    def i(self, n=16):
        t = (torch.arange(n, dtype=torch.float32) / 8 - 0.75).to(self.in_dtype).cuda()  # exact in fp16 and bf16
        self.keep.append(t)
        return t.data_ptr()

    def o(self, n=16, dtype=torch.float32):
        t = torch.full((n,), SENTINEL, dtype=dtype, device="cuda")
        self.outs.append(t)
        return t.data_ptr()

    def idx(self, n=2, out=False):
        t = torch.full((n,), 77 if out else 0, dtype=torch.int64, device="cuda")
        (self.outs if out else self.keep).append(t)
        return t.data_ptr()

    def i32(self, vals):
        t = torch.tensor(vals, dtype=torch.int32, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == (77 if t.dtype == torch.int64 else SENTINEL)).all()) for t in self.outs)


def _resize_desc(k):
    d = nat.GmResizeDesc()
    for a, n in enumerate((1, 1, 2)):
        d.n_in[a] = d.n_out[a] = n
        d.start[a] = k.i32(list(range(n + 1)))
        d.index[a] = k.i32(list(range(n)))
        d.weight[a] = k.i(n)
    k.keep.append(d)
    return C.byref(d)


def _taps(n):
    return (C.c_float * n)(*([1.0 / n] * n))


# name[:variant] -> call(L, k, d, n): d = the dtype code under test, n = 0 for the empty problem, else the batch / row / element count given
# SPECS[name] = (call, n of the 16-element problem, return value of the empty problem with a dtype that is not served)
SPECS = {
    "gm_sched_step": (lambda L, k, d, n: L.gm_sched_step(k.i(), k.i(), None, k.o(), None, n, 16, 16, d, C.byref(nat.GmStepParams()), k.s), 1, 0),
    "gm_lincomb": (lambda L, k, d, n: L.gm_lincomb((C.c_void_p * 4)(k.i(), None, None, None), (C.c_float * 4)(1, 0, 0, 0), 1, 1.0, 1.0, k.o(), n, d, k.s), 16, 0),
    "gm_likelihood_term": (lambda L, k, d, n: L.gm_likelihood_term(k.i(), k.i(), k.i(), k.o(), k.o(), k.o(16, torch.float64), n, 16, 16, d,
                                                                   C.byref(nat.GmKlParams()), k.s), 1, 0),
    "gm_axpby_rows": (lambda L, k, d, n: L.gm_axpby_rows(k.i(), k.i(), k.i(), k.i(), k.o(), n, 16, d, k.s), 1, 0),
    "gm_copy_channels:src": (lambda L, k, d, n: L.gm_copy_channels(k.i(), 5, d, k.o(), 5, F32, n, 5, k.s), 3, 0),
    "gm_copy_channels:dst": (lambda L, k, d, n: L.gm_copy_channels(k.i(), 5, F32, k.o(), 5, d, n, 5, k.s), 3, 0),
    "gm_copy_channels:both": (lambda L, k, d, n: L.gm_copy_channels(k.i(), 5, d, k.o(), 5, d, n, 5, k.s), 3, 0),
    "gm_nchw_to_nhwc:src": (lambda L, k, d, n: L.gm_nchw_to_nhwc(k.i(), d, k.o(), BF16, n, 4, 4, 4, k.s), 1, 0),
    "gm_nchw_to_nhwc:dst": (lambda L, k, d, n: L.gm_nchw_to_nhwc(k.i(), BF16, k.o(), d, n, 4, 4, 4, k.s), 1, 0),
    "gm_nhwc_to_nchw:src": (lambda L, k, d, n: L.gm_nhwc_to_nchw(k.i(), 4, d, k.o(), F32, n, 4, 4, k.s), 1, 0),
    "gm_nhwc_to_nchw:dst": (lambda L, k, d, n: L.gm_nhwc_to_nchw(k.i(), 4, F32, k.o(), d, n, 4, 4, k.s), 1, 0),
    "gm_resample2x": (lambda L, k, d, n: L.gm_resample2x(k.i(), 1, k.o(), 1, n, 1, 1, 2, 2, 0, 0, d, k.s), 1, 0),
    "gm_phase2x": (lambda L, k, d, n: L.gm_phase2x(k.i(), 1, k.o(), 1, n, 1, 1, 4, 4, 0, 0, d, k.s), 1, 0),
    "gm_timestep_embedding": (lambda L, k, d, n: L.gm_timestep_embedding(k.i(), k.o(), n, 8, 10000.0, d, k.s), 2, 0),
    "gm_geglu": (lambda L, k, d, n: L.gm_geglu(k.i(), 8, k.o(), 4, n, 4, d, k.s), 2, 0),
    "gm_aekl_sample": (lambda L, k, d, n: L.gm_aekl_sample(k.i(), k.i(), k.i(), k.o(), k.o(), n, d, k.s), 16, 0),
    "gm_addcmul": (lambda L, k, d, n: L.gm_addcmul(k.i(), k.i(), k.i(), k.o(), n, d, k.s), 16, 0),
    "gm_scale": (lambda L, k, d, n: L.gm_scale(k.i(), k.o(), 2.0, 0, n, d, k.s), 16, 0),
    "gm_activation": (lambda L, k, d, n: L.gm_activation(k.i(), None, k.o(), 1, 0, n, d, k.s), 16, 0),
    "gm_nearest_resize": (lambda L, k, d, n: L.gm_nearest_resize(k.i(), 1, k.o(), 1, n, 1, 2, 2, 1, 4, 4, 1, d, k.s), 1, 0),
    "gm_gn_scale_shift": (lambda L, k, d, n: L.gm_gn_scale_shift(k.i(), 8, n, 2, 8, 2, 1e-5, None, None, k.o(), k.o(), None, None, k.o(1024), d, k.s), 1, 0),
    "gm_gn_channel_stats": (lambda L, k, d, n: L.gm_gn_channel_stats(k.i(), 8, n, 2, 8, k.o(16, torch.float64), d, k.s), 1, 0),
    "gm_gn_apply": (lambda L, k, d, n: L.gm_gn_apply(k.i(), 8, k.o(), 8, k.i(), k.i(), 8, n, 2, 8, 1, d, k.s), 1, 0),
    "gm_spade_apply": (lambda L, k, d, n: L.gm_spade_apply(k.i(), 8, k.o(), 8, k.i(), k.i(), 8, k.i(), k.i(), 8, n, 2, 8, 1, d, k.s), 1, 0),
    "gm_layernorm": (lambda L, k, d, n: L.gm_layernorm(k.i(), 8, k.o(), 8, None, None, n, 8, 1e-5, d, k.s), 2, 0),
    "gm_gn_bwd_stats": (lambda L, k, d, n: L.gm_gn_bwd_stats(k.i(), 8, k.i(), 8, k.i(), k.i(), 8, n, 2, 8, 1, k.o(16, torch.float64), d, k.s), 1, 0),
    "gm_gn_bwd_apply": (lambda L, k, d, n: L.gm_gn_bwd_apply(k.i(), 8, k.i(), 8, k.o(), 8, k.i(), k.i(), 8, k.i(), k.i(), k.i(), n, 2, 8, 1, d, k.s), 1, 0),
    "gm_spade_bwd": (lambda L, k, d, n: L.gm_spade_bwd(k.i(), 8, k.i(), k.i(), 8, k.i(), 8, k.o(), 8, k.o(), k.o(), 8, n, 8, 1, d, k.s), 2, 0),
    "gm_layernorm_bwd": (lambda L, k, d, n: L.gm_layernorm_bwd(k.i(), 8, k.i(), 8, k.o(), 8, None, n, 8, 1e-5, None, d, k.s), 2, 0),
    "gm_geglu_bwd": (lambda L, k, d, n: L.gm_geglu_bwd(k.i(), 8, k.i(), 4, k.o(), 8, n, 4, d, k.s), 2, 0),
    "gm_embed_tokens": (lambda L, k, d, n: L.gm_embed_tokens(k.idx(), k.i(), k.i(), k.o(), n, 2, 8, 0, 2, 2, d, k.s), 1, 0),
    "gm_embed_positions_grad": (lambda L, k, d, n: L.gm_embed_positions_grad(k.i(), k.o(), n, 2, 8, 2, d, k.s), 1, -2),  # (no batch: the table is zeroed)
    "gm_sample_probs": (lambda L, k, d, n: L.gm_sample_probs(k.i(), 8, k.o(), n, 8, 1.0, 0, 0, d, k.s), 2, 0),
    "gm_token_log_prob": (lambda L, k, d, n: L.gm_token_log_prob(k.i(), 8, k.idx(), k.o(), n, 8, d, k.s), 2, 0),
    "gm_spade_block_apply": (lambda L, k, d, n: L.gm_spade_block_apply(k.i(), 8, k.i(), k.i(), 8, None, None, 0, k.o(), 8, None, None, 0, None, 0, n, 1, 1, 2,
                                                                       1, 1, 2, 8, 0, 0, 0.2, d, k.s), 1, 0),
    "gm_leaky_relu": (lambda L, k, d, n: L.gm_leaky_relu(k.i(), None, k.o(), 0.2, n, d, k.s), 16, 0),
    "gm_kld": (lambda L, k, d, n: L.gm_kld(k.i(), k.i(), n, k.o(), None, None, None, d, k.s), 16, -2),  # (no elements: the loss is 0, and is written)
    "gm_vq_argmin": (lambda L, k, d, n: L.gm_vq_argmin(k.i(), 8, k.i(), k.idx(2, out=True), n, 2, 8, d, k.s), 2, 0),
    "gm_vq_gather": (lambda L, k, d, n: L.gm_vq_gather(k.idx(), k.i(), k.o(), 8, None, 0, None, None, n, 2, 8, d, k.s), 2, 0),
    "gm_vq_ema_stats": (lambda L, k, d, n: L.gm_vq_ema_stats(k.i(), 8, k.idx(), n, 2, 8, k.o(32), k.o(64), d, k.s), 2, -2),  # (no tokens: zeros are written)
    "gm_resize_taps": (lambda L, k, d, n: L.gm_resize_taps(k.i(), 8, k.o(), 8, n, 8, _resize_desc(k), d, k.s), 1, -2),  # (refuses before it looks at the size)
    # the metric entry points reject an empty input as an argument error, before the dtype
    "gm_ssim_cs": (lambda L, k, d, n: L.gm_ssim_cs(k.i(), k.i(), d, n, 1, 1, 4, 4, _taps(1), 1, _taps(3), 3, _taps(3), 3, 1e-4, 9e-4, k.o(), k.o(), None, None,
                                                   k.o(1024), 4096, k.s), 1, -1),
    "gm_avgpool2_pair": (lambda L, k, d, n: L.gm_avgpool2_pair(k.i(), k.i(), d, k.o(), k.o(), n, 1, 4, 4, 0, k.s), 1, -1),
    "gm_mmd": (lambda L, k, d, n: L.gm_mmd(k.i(), k.i(), d, n, 8, k.o(), k.o(1024), 4096, k.s), 2, -1),
}
METRICS = ("gm_ssim_cs", "gm_avgpool2_pair", "gm_mmd")
WHERE = {"gm_embed_tokens": "gm_embed_tokens_dev"}  # (the entry point whose body refuses)


def _refused(name, d):
    L = nat.lib()
    call, n, _ = SPECS[name]
    assert L.gm_scale(None, None, 1.0, 0, 1, F32, None) == -1  # a different message into the error slot
    k = Ctx()
    rc = call(L, k, d, n)
    entry = name.split(":")[0]
    assert rc == -2, f"{name} with dtype {d}: returned {rc} ({L.gm_last_error()})"
    assert L.gm_last_error() == f"{WHERE.get(entry, entry)}: error -2: unsupported dtype".encode()
    assert k.untouched(), f"{name} with dtype {d}: an output changed"


@pytest.mark.parametrize("name", sorted(SPECS))
def test_unknown_dtype_is_refused(name):
    _refused(name, BAD)


@pytest.mark.parametrize("name", sorted(n for n in SPECS if n not in METRICS))
def test_fp16_is_refused_outside_the_metrics(name):
    _refused(name, F16)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_empty_problem_before_the_dtype(name):
    L = nat.lib()
    call, _, want = SPECS[name]
    k = Ctx()
    rc = call(L, k, BAD, 0)
    assert rc == want, f"{name}, empty problem with dtype {BAD}: returned {rc}, expected {want} ({L.gm_last_error()})"
    assert k.untouched()


@pytest.mark.parametrize("name", METRICS)
def test_metrics_serve_fp16(name):
    L = nat.lib()
    call, n, _ = SPECS[name]
    got = {}
    for d, tdt in ((F32, torch.float32), (F16, torch.float16)):
        k = Ctx(tdt)
        rc = call(L, k, d, n)
        assert rc == 0, f"{name} with dtype {d}: returned {rc} ({L.gm_last_error()})"
        torch.cuda.synchronize()
        got[d] = [t.clone() for t in k.outs[:2 if name != "gm_mmd" else 1]]  # (the workspace behind them holds partials)
    for a, b in zip(got[F32], got[F16]):
        nres = 1 if name != "gm_avgpool2_pair" else 4
        assert bool((a[:nres] != SENTINEL).all()), f"{name}: no result written"
        assert torch.equal(a, b), f"{name}: fp16 inputs (exact values) give {b[:nres].tolist()}, fp32 gives {a[:nres].tolist()}"
