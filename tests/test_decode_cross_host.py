"""CPU (-m "not gpu"): the cross-attention stage of the transformer decode step, on the host alone.
  * gm_decode_cross_route (the function gm_transformer_decode_step itself consults) pinned over the matrix tests/test_gpu_decode_cross.py runs on the GPU,
    with its refusals; the twelve plan flags do not depend on the context length;
  * the sharpness conditions of that GPU test shown with the fp64 reference alone (tests/_decode_cross_ref.py), over the whole matrix, both dtypes and
    every position: masking the first or the last context key, swapping the samples' contexts, or dropping the cross stage moves the logits by at
    least 4x the bar."""
import ctypes as C

import pytest
import torch

import _decode_cross_ref as X
from generativemodels_amd import _native

F32, BF16 = X.F32, X.BF16


def _route(d):
    return _native.lib().gm_decode_cross_route(C.byref(d))


def test_the_header_names_the_cross_routes_outside_the_plan_flags():
    assert (X.NONE, X.FUSED, X.COMPOSED) == (0, 1, 2)
    assert X.K["GM_DECODE_PLAN_COUNT"] == 12 and len([k for k in X.K if k.startswith("GM_DECODE_PLAN_")]) == 13
    assert X.K["GM_DECODE_CROSS_MAX_FUSED_CTX"] == 4096


@pytest.mark.parametrize("c,heads,window,batch,lc", X.MATRIX)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_cross_route_and_plan_of_every_matrix_entry(c, heads, window, batch, lc, dtype):
    d, keep = X.descriptor(c, heads, window, batch, dtype, lc)
    assert _route(d) == X.EXPECT[(c, heads, window, batch, lc)]
    # neither the position's source nor the depth changes the route
    assert _route(X.descriptor(c, heads, window, batch, dtype, lc, device_pos=True)[0]) == X.EXPECT[(c, heads, window, batch, lc)]
    d1, keep1 = X.descriptor(c, heads, window, batch, dtype, lc, depth=1)
    assert _route(d1) == X.EXPECT[(c, heads, window, batch, lc)]
    # no context: no cross attention, and the cross fields are not looked at
    d0, keep0 = X.descriptor(c, heads, window, batch, dtype, 0)
    for b in keep0:
        b.ln2_g = b.w_cq = b.w_co = b.ck = b.cv = None
    assert _route(d0) == X.NONE
    # the twelve plan flags are those of the model without a context, with a host and with a device position
    for dev in (False, True):
        with_ctx = X.plan_flags(X.descriptor(c, heads, window, batch, dtype, lc, device_pos=dev)[0])
        assert with_ctx == X.plan_flags(X.descriptor(c, heads, window, batch, dtype, 0, device_pos=dev)[0])
    assert len(with_ctx) == 12


def test_the_matrix_reaches_both_cross_routes():
    assert len(X.EXPECT) == len(X.MATRIX)
    for dtype in (F32, BF16):
        assert {_route(X.descriptor(*e[:4], dtype, e[4])[0]) for e in X.MATRIX} == {X.FUSED, X.COMPOSED}


def test_the_context_bound_of_the_fused_kernel():
    bound = X.K["GM_DECODE_CROSS_MAX_FUSED_CTX"]
    for dtype in (F32, BF16):
        assert _route(X.descriptor(256, 8, 1000, 2, dtype, bound)[0]) == X.FUSED
        assert _route(X.descriptor(256, 8, 1000, 2, dtype, bound + 1)[0]) == X.COMPOSED
        assert _route(X.descriptor(256, 8, 1000, 16, dtype, 77)[0]) == X.FUSED
        assert _route(X.descriptor(256, 8, 1000, 17, dtype, 77)[0]) == X.COMPOSED


def test_cross_route_refusals():
    with X.last_error_kept():
        _refusals()


def _refusals():
    lib = _native.lib()
    d, keep = X.descriptor(256, 8, 1000, 2, BF16, -1)
    assert _route(d) < 0 and b"negative context length" in lib.gm_last_error()
    for field in ("ln2_g", "w_cq", "w_co", "ck", "cv"):
        for blk in range(X.DEPTH):  # a null pointer in ANY block, not only the first
            d, keep = X.descriptor(256, 8, 1000, 2, BF16, 77)
            setattr(keep[blk], field, None)
            assert _route(d) < 0, (field, blk)
            assert b"null cross-attention pointer" in lib.gm_last_error()
            d.ctx_len = 0
            assert _route(d) == X.NONE
    # the optional ones: LayerNorm2's bias, the biases of to_q and out_proj
    d, keep = X.descriptor(256, 8, 1000, 2, BF16, 77)
    for b in keep:
        b.ln2_b = b.b_cq = b.b_co = None
    assert _route(d) == X.FUSED
    assert lib.gm_decode_cross_route(None) < 0


@pytest.mark.parametrize("c,heads,window,batch,lc", X.MATRIX)
def test_the_reference_is_sensitive_to_every_planted_operand(c, heads, window, batch, lc):
    _, sd = X.build_model(c, heads, window)
    for code in (F32, BF16):
        dtype = X.DT[code]
        ref = X.CrossReference(X.params64(sd, dtype), heads)
        base = X.base_operands(c, heads, window, batch, lc, dtype)
        for p in X.positions(window):
            tok = torch.randint(0, X.VOCAB, (batch,), generator=base["g"])
            o = X.operands(ref, base, tok, p, lc, dtype, seed=p)
            # the contexts differ between the samples, and the planted keys score PLANT_SCORE against their own sample's query only
            assert not torch.equal(o["ck"][0][0], o["ck"][0][1])
            bad = X.sensitivity_failures(ref, o, tok, p, lc, dtype)
            assert not bad, f"{str(dtype)[6:]} C {c} heads {heads} window {window} B {batch} Lc {lc} p {p}: the reference is blind to " + "; ".join(bad)
