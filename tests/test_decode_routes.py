"""CPU (-m "not gpu"): the route plan of the transformer decode step (gm_transformer_decode_plan, the function gm_transformer_decode_step
itself consults) pinned over the matrix that tests/test_gpu_decode_matrix.py runs on the GPU.  Descriptors carry dummy non-null pointers:
the plan launches nothing and dereferences only the host block table."""
import ctypes as C
import os
import re

import pytest

from generativemodels_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1  # GM_F32, GM_BF16
SWITCHES = ("GM_DECODE_KV_SPLIT", "GM_DECODE_KV_FUSE", "GM_DECODE_QKV_FUSE", "GM_DECODE_MLP_FUSE", "GM_LINEAR_KSPLIT")


def _header_constants():
    src = open(os.path.join(ROOT, "include", "gm_amd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (GM_DECODE_[A-Z_]+) (\d+)", src)}


K = _header_constants()
FLAG_NAMES = sorted((k for k in K if k.startswith("GM_DECODE_PLAN_") and k != "GM_DECODE_PLAN_COUNT"), key=K.get)
SHORT = [n[len("GM_DECODE_PLAN_"):].lower() for n in FLAG_NAMES]

# (C, heads, window, batch): the matrix of the GPU test, in its order.  M = 4 C, vocabulary 50, depth 2.
MATRIX = [
    (256, 8, 1000, 2), (512, 16, 1000, 2), (128, 2, 1000, 2), (256, 4, 1000, 2), (320, 8, 1000, 2), (240, 12, 1000, 2), (232, 29, 1000, 2),
    (72, 3, 700, 2), (256, 8, 1000, 17), (256, 8, 4100, 1), (256, 8, 257, 2), (256, 8, 256, 2), (72, 3, 200, 2),
    (128, 4, 1000, 2),  # the one entry beyond the issue's table: without it no fp32 geometry reaches <float, 6, 2> (8 K chunks of 16)
]
ROW, MLPM = K["GM_DECODE_INPUT_ROW"], K["GM_DECODE_INPUT_MLP_MERGE"]
OUTP, COMB = K["GM_DECODE_MERGE_OUT_PROJ"], K["GM_DECODE_MERGE_COMBINE"]
HOST, DEVP = K["GM_DECODE_ENTRY_HOST_POS"], K["GM_DECODE_ENTRY_DEVICE_POS"]


def _p(split, ng, um, inp, merge, entry, mlp, kq, ko, ku, kd, kl):
    return dict(zip(SHORT, (split, ng, um, inp, merge, entry, mlp, kq, ko, ku, kd, kl)))


# The expected plan of every entry with a HOST position, derived by hand from the predicates of csrc/rows_gemm.hip, csrc/decode_attention.hip and csrc/decode_step.hip:
#   K-split GEMM: rows <= 16 and ceil(cin / BK) >= 8 (BK 16 fp32, 32 bf16);  fused MLP: K-split at C, C <= 512, M % 64 == 0;
#   fused q|k|v: window > 256, dh % 16 == 0, C % BK == 0, (NG, UM) = (3 dh / 16, ceil(C / BK / 4)) rounded up into {(6,2), (6,4), (12,2)};
#   partial merge in the out-projection: dh % VECW == 0 (VECW 4 fp32, 8 bf16) and the out-projection K-split.
EXPECT = {
    # everything fused: bf16 8 K chunks -> UM 2, fp32 16 -> UM 4
    (256, 8, 1000, 2, BF16): _p(1, 6, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (256, 8, 1000, 2, F32): _p(1, 6, 4, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    # bf16 16 K chunks -> <6,4>; fp32 32 chunks -> UM 8: no instantiation, MLP-merge + LN K-split GEMM, split attention, kvmerge
    (512, 16, 1000, 2, BF16): _p(1, 6, 4, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (512, 16, 1000, 2, F32): _p(1, 0, 0, MLPM, OUTP, 0, 1, 1, 1, 0, 0, 1),
    # dh 64 -> NG 12.  bf16: 4 K chunks, no K-split GEMM: plain row, combine launch, unfused MLP (its M = 512 down-projection is K-split)
    (128, 2, 1000, 2, BF16): _p(1, 12, 2, ROW, COMB, 0, 0, 0, 0, 0, 1, 0),
    (128, 2, 1000, 2, F32): _p(1, 12, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    # bf16 <12,2> behind a fused MLP; fp32 16 chunks -> UM 4 with NG 12: falls back
    (256, 4, 1000, 2, BF16): _p(1, 12, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (256, 4, 1000, 2, F32): _p(1, 0, 0, MLPM, OUTP, 0, 1, 1, 1, 0, 0, 1),
    # dh 40: never fused, kvmerge in both dtypes
    (320, 8, 1000, 2, BF16): _p(1, 0, 0, MLPM, OUTP, 0, 1, 1, 1, 0, 0, 1),
    (320, 8, 1000, 2, F32): _p(1, 0, 0, MLPM, OUTP, 0, 1, 1, 1, 0, 0, 1),
    # dh 20: bf16 scalar key/value path -> combine launch, K-split GEMM with a ragged last chunk (240 % 32); fp32 vector path
    (240, 12, 1000, 2, BF16): _p(1, 0, 0, MLPM, COMB, 0, 1, 1, 1, 0, 0, 1),
    (240, 12, 1000, 2, F32): _p(1, 0, 0, MLPM, OUTP, 0, 1, 1, 1, 0, 0, 1),
    # M = 928, M % 64 != 0: K-split projections around an unfused MLP
    (232, 29, 1000, 2, BF16): _p(1, 0, 0, ROW, OUTP, 0, 0, 1, 1, 1, 1, 1),
    (232, 29, 1000, 2, F32): _p(1, 0, 0, ROW, OUTP, 0, 0, 1, 1, 1, 1, 1),
    # C = 72: no projection from C is K-split, fully unfused (only the M = 288 down-projection has 8 K chunks or more)
    (72, 3, 700, 2, BF16): _p(1, 0, 0, ROW, COMB, 0, 0, 0, 0, 0, 1, 0),
    (72, 3, 700, 2, F32): _p(1, 0, 0, ROW, COMB, 0, 0, 0, 0, 0, 1, 0),
    # 17 rows: fused q|k|v with plain-row input, no K-split anywhere
    (256, 8, 1000, 17, BF16): _p(1, 6, 2, ROW, COMB, 0, 0, 0, 0, 0, 0, 0),
    (256, 8, 1000, 17, F32): _p(1, 6, 4, ROW, COMB, 0, 0, 0, 0, 0, 0, 0),
    # windows 4100 (key ranges of 320) and 257 (the smallest split window): the routes of the first entry
    (256, 8, 4100, 1, BF16): _p(1, 6, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (256, 8, 4100, 1, F32): _p(1, 6, 4, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (256, 8, 257, 2, BF16): _p(1, 6, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    (256, 8, 257, 2, F32): _p(1, 6, 4, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    # fp32 <6,2>: 8 K chunks of 16 (bf16: 4 chunks, <6,2> again, nothing K-split from C)
    (128, 4, 1000, 2, BF16): _p(1, 6, 2, ROW, COMB, 0, 0, 0, 0, 0, 1, 0),
    (128, 4, 1000, 2, F32): _p(1, 6, 2, MLPM, OUTP, 0, 1, 0, 1, 0, 0, 1),
    # not split
    (256, 8, 256, 2, BF16): _p(0, 0, 0, MLPM, 0, HOST, 1, 1, 1, 0, 0, 1),
    (256, 8, 256, 2, F32): _p(0, 0, 0, MLPM, 0, HOST, 1, 1, 1, 0, 0, 1),
    (72, 3, 200, 2, BF16): _p(0, 0, 0, ROW, 0, HOST, 0, 0, 0, 0, 1, 0),
    (72, 3, 200, 2, F32): _p(0, 0, 0, ROW, 0, HOST, 0, 0, 0, 0, 1, 0),
}


def plan_of(c, heads, window, batch, dtype, device_pos=False, depth=2):
    """The plan of a depth-`depth` model of width c (M = 4 c, vocabulary 50) as {short flag name: value}; dummy pointers throughout."""
    dummy = 0x1000
    blocks = (_native.GmDecodeBlock * depth)()
    for b in blocks:
        for name, _ in _native.GmDecodeBlock._fields_:
            setattr(b, name, dummy)
        b.b_qkv = None  # (qkv_bias = False)
    d = _native.GmDecodeDesc()
    d.B, d.C, d.M, d.heads, d.depth, d.max_len, d.num_tokens, d.dtype = batch, c, 4 * c, heads, depth, window, 50, dtype
    d.ln_eps, d.pos = 1e-5, 0
    for name in ("tokens", "tok_emb", "pos_emb", "w_logits", "b_logits", "logits", "scratch"):
        setattr(d, name, dummy)
    d.blocks = blocks
    d.scratch_bytes = _native.lib().gm_decode_scratch_bytes(batch, c, 4 * c, dtype)
    d.pos_dev = dummy if device_pos else None
    flags = (C.c_int * K["GM_DECODE_PLAN_COUNT"])()
    _native.check(_native.lib().gm_transformer_decode_plan(C.byref(d), flags), "gm_transformer_decode_plan")
    return {s: flags[K[n]] for s, n in zip(SHORT, FLAG_NAMES)}


def describe(plan):
    return " ".join(f"{k}={v}" for k, v in plan.items())


def test_no_bench_switch_is_set():
    assert not [s for s in SWITCHES if os.environ.get(s) is not None]


def test_the_header_names_every_plan_flag_once():
    assert [K[n] for n in FLAG_NAMES] == list(range(K["GM_DECODE_PLAN_COUNT"])) and K["GM_DECODE_PLAN_COUNT"] == 12


@pytest.mark.parametrize("c,heads,window,batch", MATRIX)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_plan_of_every_matrix_entry(c, heads, window, batch, dtype):
    want = EXPECT[(c, heads, window, batch, dtype)]
    got = plan_of(c, heads, window, batch, dtype)
    assert got == want, f"got  {describe(got)}\nwant {describe(want)}"
    # a device position changes the non-split attention entry and nothing else
    dev = plan_of(c, heads, window, batch, dtype, device_pos=True)
    want_dev = dict(want, attn_entry=DEVP if want["attn_entry"] == HOST else want["attn_entry"])
    assert dev == want_dev, describe(dev)
    # block 0 has no MLP partials in front of it: a depth-1 model reads the plain row, everything else as above
    assert plan_of(c, heads, window, batch, dtype, depth=1) == dict(want, qkv_input=ROW)


def test_the_matrix_reaches_every_value_of_every_flag_and_every_fused_instantiation():
    plans = {(e, dt, dev): plan_of(*e, dt, device_pos=dev) for e in MATRIX for dt in (F32, BF16) for dev in (False, True)}
    assert len(EXPECT) == 2 * len(MATRIX)
    values = {
        "split_kv": {0, 1}, "qkv_ng": {0, 6, 12}, "qkv_um": {0, 2, 4}, "qkv_input": {ROW, MLPM}, "out_merge": {0, OUTP, COMB},
        "attn_entry": {0, HOST, DEVP}, "mlp_fused": {0, 1}, "ksplit_qkv": {0, 1}, "ksplit_out": {0, 1}, "ksplit_mlp_up": {0, 1},
        "ksplit_mlp_down": {0, 1}, "ksplit_logits": {0, 1},
    }
    assert sorted(values) == sorted(SHORT)
    for flag, want in values.items():
        assert {p[flag] for p in plans.values()} == want, flag
    for dt in (F32, BF16):
        inst = {(p["qkv_ng"], p["qkv_um"]) for (e, d, dev), p in plans.items() if d == dt}
        assert inst == {(0, 0), (6, 2), (6, 4), (12, 2)}, (dt, inst)
        # the fused kernel both behind a fused MLP (partial-merging input) and without one (plain row)
        assert {p["qkv_input"] for (e, d, dev), p in plans.items() if d == dt and p["qkv_ng"]} == {ROW, MLPM}
        # the unfused q|k|v GEMM in both input forms, and both merges behind both q|k|v forms
        assert {p["qkv_input"] for (e, d, dev), p in plans.items() if d == dt and p["split_kv"] and not p["qkv_ng"]} == {ROW, MLPM}
        assert {(bool(p["qkv_ng"]), p["out_merge"]) for (e, d, dev), p in plans.items() if d == dt and p["split_kv"]} == \
            {(True, OUTP), (True, COMB), (False, OUTP), (False, COMB)}

