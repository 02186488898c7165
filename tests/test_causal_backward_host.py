"""CPU: the host side of the causal attention backward (csrc/attention_bwd.hip, CAUSAL) -- the tile walk its kernels run, against a brute-force
visibility matrix; the "causal" row of the route table; and that the operands of tests/test_gpu_causal_backward.py would expose a mask that is
off by one key."""
import ctypes
import gzip
import json
import os

import pytest
import torch

import _causal_ref as CR
from _util import GOLDEN

OWN, TILE = 64, 32  # own rows of a work-group, rows of a streamed tile
OFFS = (0, 1, 31, 32, 33, 37, 64, 100)


def _walk(lib, lq, lk, block):
    ke, qb = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.gm_attention_backward_causal_walk(lq, lk, block, ctypes.byref(ke), ctypes.byref(qb)) == 0
    return ke.value, qb.value


def test_walk_streams_exactly_the_tiles_that_hold_a_visible_pair():
    """gm_attention_backward_causal_walk -- the two inline functions the kernels call -- for every Lq in 1 .. 200, every offset and every block:
    the key tiles [0, key_end) are exactly those with a (query of the block, key of the tile) pair inside the mask, the query tiles
    [query_begin, Lq) exactly those with a (query of the tile, key of the block) pair inside it."""
    from generativemodels_amd import _native
    lib = _native.lib()
    for off in OFFS:
        for lq in range(1, 201):
            lk = lq + off
            vis = torch.arange(lk)[None, :] <= torch.arange(lq)[:, None] + off  # [query][key]
            for block in range((lq + OWN - 1) // OWN):
                key_end, _ = _walk(lib, lq, lk, block)
                mine = vis[block * OWN:(block + 1) * OWN]
                want = [k0 for k0 in range(0, lk, TILE) if mine[:, k0:k0 + TILE].any()]
                assert 0 < key_end <= lk and list(range(0, key_end, TILE)) == want, (lq, off, block, key_end)
            for block in range((lk + OWN - 1) // OWN):
                _, q_begin = _walk(lib, lq, lk, block)
                mine = vis[:, block * OWN:(block + 1) * OWN]
                want = [q0 for q0 in range(0, lq, TILE) if mine[q0:q0 + TILE].any()]
                assert 0 <= q_begin < lq and q_begin % TILE == 0 and list(range(q_begin, lq, TILE)) == want, (lq, off, block, q_begin)


def test_walk_refuses_what_the_kernels_do_not_serve():
    from generativemodels_amd import _native
    lib = _native.lib()
    ke, qb = ctypes.c_int(), ctypes.c_int()
    for lq, lk, block in ((0, 4, 0), (5, 4, 0), (4, 4, -1)):
        assert lib.gm_attention_backward_causal_walk(lq, lk, block, ctypes.byref(ke), ctypes.byref(qb)) != 0
    assert lib.gm_attention_backward_causal_walk(4, 4, 0, None, ctypes.byref(qb)) != 0
    assert _walk(lib, 10, 100, 1) == (0, 0)     # no queries in block 1; its keys 64 .. 99 are seen from query 0 on
    assert _walk(lib, 10, 100, 2) == (0, 10)    # neither queries nor keys


def test_causal_route_for_every_dtype_and_length():
    from generativemodels_amd import autograd as A
    route = A.attention_backward_route
    for dt in (torch.float32, torch.bfloat16):
        for b, h, lq, lk in ((1, 1, 1, 1), (2, 8, 65, 65), (1, 8, 4096, 4096), (2, 3, 70, 170), (1, 1, 32768, 32768), (4, 8, 9000, 9000)):
            for dh, dhp in ((8, 16), (12, 16), (16, 16), (24, 32), (40, 64), (64, 64), (256, 256)):
                assert route(dt, b, h, lq, lk, dh, causal=True) == ("causal", dhp)
                assert route(dt, b, h, lq, lk, dh, fused=False, causal=True) == ("causal", dhp)
        with pytest.raises(ValueError, match="head dims up to 256"):
            route(dt, 1, 2, 65, 65, 300, causal=True)


def test_route_table_without_the_mask_still_reads_like_the_committed_golden():
    """causal defaults to False: the routes of the golden launch census (tests/golden/attention_routes.json.gz) are what the table answers."""
    from generativemodels_amd import autograd as A
    with gzip.open(os.path.join(GOLDEN, "attention_routes.json.gz"), "rt") as fh:
        cases = json.load(fh)["cases"]
    entry = {"gm_attention_backward_fused": "fused", "gm_attention_bwd_scores": "bf16", "gm_attention_backward": "flash"}
    seen = set()
    for cid, recs in cases.items():
        c = json.loads(cid)
        if c["kind"] != "autograd" or c.get("declined") or recs[0][0] == "raise":
            continue
        launched = [entry[r[0]] for r in recs if r[0] in entry]
        want = launched[0] if launched else "composed"
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[c["dtype"]]
        args = (dt, c["b"], c["heads"], c["lq"], c["lk"], c["dh"])
        assert A.attention_backward_route(*args)[0] == want == A.attention_backward_route(*args, causal=False)[0], cid
        seen.add(want)
    assert seen == {"fused", "bf16", "flash", "composed"}


# (Lq, Lk, dh) at B 2, H 3: tests/test_gpu_causal_backward.py runs its peaked operands at these
SENSITIVITY_SHAPES = [(33, 33, 16), (65, 65, 16), (65, 65, 64), (129, 129, 32), (300, 300, 32), (129, 166, 64), (70, 170, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SENSITIVITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_peaked_operands_expose_a_mask_that_is_off_by_one_key(shape, dtype):
    """A kernel whose mask is one key too wide or too narrow must fail the GPU test: over the diagonal-peaked operands, the fp64 gradients under
    the shifted mask leave the bar of the tested dtype in at least 90 % of the rows of each of dq, dk, dv.  (Measured: >= 92 % everywhere; randn
    operands alone fall to about a third of the rows under the bf16 bar, which is why the GPU test does not rely on them.)"""
    lq, lk, dh = shape
    b, h = 2, 3
    q, k, v, go = CR.operands("peaked", dtype, b, h, lq, lk, dh, seed=7)
    scale = 1.0 / dh ** 0.5
    want = CR.reference(q, k, v, go, h, scale)
    for shift in (+1, -1):
        wrong = CR.reference(q, k, v, go, h, scale, shift=shift)
        for name, g, w in zip(("dq", "dk", "dv"), wrong[1:], want[1:]):
            over = (CR.row_ratios(g, w, CR.BARS[dtype]) > 1.0).double().mean().item()
            print(f"{shape} {dtype} shift {shift:+d} {name}: {over:.3f} of the rows over the bar")
            assert over >= 0.90, (name, shift, over)
