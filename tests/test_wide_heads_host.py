"""CPU: attention heads wider than 256 channels -- the library's wide-head entry point, the oracle at the reference's real widths
(tests/golden/wide_nets.pt, made by tools/make_golden_wide.py from the unmodified reference), and the backward routing for wide heads."""
import os

import pytest
import torch

import restatement as R
from _util import GOLDEN, assert_close

WIDE = "wide_nets"


def test_library_exports_the_wide_head_limit():
    from generativemodels_amd import _native
    lib = _native.lib()
    assert lib.gm_attention_max_wide_head_dim() >= 1024
    assert lib.gm_attention_max_head_dim() == 256  # the single-pass kernels' bound is unchanged


def _case(name):
    fx = torch.load(os.path.join(GOLDEN, WIDE + ".pt"), weights_only=False)
    c = fx["cases"][name]
    return c, R.synthetic_state_dict(c["shapes"], seed=c["synthetic_seed"])


@pytest.mark.parametrize("name", ["brain", "tutorial", "cxr"])
def test_oracle_reproduces_the_wide_unets(name):
    c, sd = _case(name)
    i = c["inputs"]
    with torch.no_grad():
        for t, want in zip(i["timesteps"], c["outputs"]["y"]):
            y = R.unet_forward(sd, c["cfg"], i["x"], torch.tensor([t]), i["context"])
            assert_close(y, want, atol=2e-5 * max(1.0, want.abs().max().item()), what=f"{name} t={t}")


def test_oracle_reproduces_the_wide_autoencoder():
    c, sd = _case("aekl")
    o = c["outputs"]
    with torch.no_grad():
        mu, sigma = R.aekl_encode(sd, c["cfg"], c["inputs"]["x"])
        rec = R.aekl_decode(sd, c["cfg"], o["z_mu"])
    assert_close(mu, o["z_mu"], 2e-5, what="z_mu")
    assert_close(sigma, o["z_sigma"], 2e-5, what="z_sigma")
    assert_close(rec, o["reconstruction"], 2e-5 * max(1.0, o["reconstruction"].abs().max().item()), what="reconstruction")


class _Ctx:
    def __init__(self, tensors, heads):
        self.saved_tensors, self.cfg = tensors, (heads, 0.05)


@pytest.mark.parametrize("dh", [320, 512, 768])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_heads_train_through_the_composed_backward(dh, dtype, monkeypatch):
    """Host routing only (meta tensors, no device): a head wider than 256 is not the fused kernels' and goes unpadded to the composed
    per-(sample, head) path; beyond ATTENTION_BWD_MAX_TOKENS it raises with the bound."""
    from generativemodels_amd import autograd as A
    heads = 2
    q = torch.empty((1, 4096, heads * dh), dtype=dtype, device="meta")
    k = torch.empty((1, 300, heads * dh), dtype=dtype, device="meta")
    assert not A._fused_backward_serves(q, k, heads)
    assert A.attention_backward_route(dtype, 1, heads, 4096, 300, dh) == ("composed", dh)  # not a fused / flash / bf16 route, and no padding
    seen = []
    monkeypatch.setattr(A, "_attention_backward_composed", lambda q_, k_, v_, go_, h_, s_: seen.append((tuple(q_.shape), h_)) or (q_, k_, v_))
    grads = A._Attention.backward(_Ctx((q, k, k, q), heads), q)
    assert seen == [((1, 4096, heads * dh), heads)] and grads[3] is None and grads[4] is None
    long_q = torch.empty((1, A.ATTENTION_BWD_MAX_TOKENS + 1, heads * dh), dtype=dtype, device="meta")
    with pytest.raises(ValueError, match=str(A.ATTENTION_BWD_MAX_TOKENS)):
        A.attention_backward_route(dtype, 1, heads, A.ATTENTION_BWD_MAX_TOKENS + 1, 300, dh)
    with pytest.raises(ValueError, match=str(A.ATTENTION_BWD_MAX_TOKENS)):
        A._Attention.backward(_Ctx((long_q, k, k, long_q), heads), long_q)
