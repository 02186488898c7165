"""CPU witness of the weight-gradient matrix: the native planner (gm_conv_wgrad_workspace_bytes, which runs without a GPU) against the restatement in
_wgrad_cases.py, for every case of the table -- and every case against the regime its label names, so that the GPU matrix cannot drift out of the split
regimes it was built for when the planner changes."""
import ctypes as C

import pytest

import _wgrad_cases as W


def _desc(case, **over):
    from generativemodels_amd import _native as nat

    (kd, kh, kw), src, out, pad = W.geometry(case)
    d = nat.GmWgradDesc()
    vals = dict(N=case.n, Cin=case.cin, Cout=case.cout, Ds=src[0], Hs=src[1], Ws=src[2], Do=out[0], Ho=out[1], Wo=out[2], kd=kd, kh=kh, kw=kw,
                stride=case.stride, pd=pad[0], ph=pad[1], pw=pad[2], dtype=W.DT_CODE[case.dtype], accumulate=0,
                x_ld=case.cin + W.VECW[case.dtype], gy_ld=case.cout + 2 * W.VECW[case.dtype], x=0x1000, gy=0x2000)
    vals.update(over)
    for k, v in vals.items():
        setattr(d, k, v)
    return d


def _bytes(case, **over):
    from generativemodels_amd import _native as nat

    return nat.lib().gm_conv_wgrad_workspace_bytes(C.byref(_desc(case, **over)))


def _check_plan(case):
    plan = W.expected_plan(case)
    got = _bytes(case)
    assert got > 0, f"{case.dtype}-{case.name}: the planner rejects the case"
    per_split = 4 * plan.kd * plan.nt * plan.ncob * 64 * plan.ncib * W.CIB[case.dtype]
    assert got % per_split == 0
    assert got // per_split == plan.nsplit, f"{case.dtype}-{case.name}: nsplit {got // per_split}, expected {plan.nsplit}"
    assert got == plan.workspace_bytes <= 36 << 20
    assert W.in_regime(plan, case.regime), f"{case.dtype}-{case.name} is labelled '{case.regime}': {plan}"
    assert [r for r in W.REGIMES if W.in_regime(plan, r)] == [case.regime], "the regimes are disjoint"
    return plan


@pytest.mark.parametrize("cid", list(W.BY_ID))
def test_every_case_is_in_the_regime_its_label_names(cid):
    case = W.BY_ID[cid]
    plan = _check_plan(case)
    assert plan.share_min in (plan.share_max, plan.share_max - 1) and plan.share_min >= 1
    voxels = case.n * W.math.prod(case.out)
    assert 4 * voxels + 4096 < 1 << 24, "integer operands in [-2, 2] and a prefill below 4096 stay exact in fp32"


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(W.CONVT))
def test_conv_transpose_cases_walk_with_the_large_operand_in_the_x_role(name, dtype):
    case = W.convt_launch(name, dtype)
    _check_plan(case)
    assert W.math.prod(case.src) >= W.math.prod(case.out)


def test_the_hand_computed_plans_of_the_issue():
    plans = {cid: W.expected_plan(c) for cid, c in W.BY_ID.items()}
    p = plans["bf16-walk3d"]
    assert (p.variant, p.tiles, p.nsplit, p.share_max, p.share_min) == (0, 27, 5, 6, 5) and plans["fp32-walk3d"].nsplit == 2
    p = plans["bf16-walk3d-n3"]
    assert p.tiles == 24 and "n" in p.carries
    p = plans["bf16-many-splits"]
    assert (p.tiles, p.nsplit, p.step, p.share_max, p.share_min, p.nsplit % 8) == (120, 85, (1, 1, 4, 0), 2, 1, 5)
    assert (plans["bf16-walk2d"].variant, plans["bf16-walk2d"].tiles, plans["bf16-walk2d"].nsplit, plans["fp32-walk2d"].nsplit) == (1, 18, 16, 8)
    assert plans["bf16-walk-s2-3d"].variant == plans["bf16-walk-s2-2d"].variant == 2 and plans["bf16-flat-walk"].variant == 3
    assert (plans["bf16-flat-cap"].nsplit, plans["bf16-flat-cap"].tiles) == (256, 274)
    assert (plans["bf16-one-split-512"].base, plans["fp32-one-split-512"].base) == (192, 384)   # fp32: 256 / 384 = 0, clamped to 1
    assert plans["bf16-one-split-512"].nsplit == plans["fp32-one-split-512"].nsplit == 1


def test_the_table_covers_every_regime_variant_and_reduction_shape_in_both_dtypes():
    for dtype in ("bf16", "fp32"):
        cases = [c for c in W.CASES if c.dtype == dtype]
        plans = [W.expected_plan(c) for c in cases]
        regimes = {c.regime for c in cases}
        assert regimes == set(W.REGIMES), dtype
        for variant in range(4):
            assert any(p.variant == variant and p.share_max == 1 for p in plans), f"{dtype}: variant {variant}, one tile per work-group"
            assert any(p.variant == variant and p.share_max >= 2 for p in plans), f"{dtype}: variant {variant} walking"
        walkers = [p for p in plans if p.share_max >= 2]
        assert any(p.share_min != p.share_max for p in walkers), "uneven tile shares"
        assert {"th", "td", "n"} <= set().union(*[p.carries for p in walkers]), "carries into th, td and n on a step that loads a tile"
        # wgrad_reduce_kernel: more elements than one pass of its capped grid; slice counts below 8, whole eights and eights with a tail
        assert any(c.cout * c.cin * p.kd * p.nt > 4096 * 256 for c, p in zip(cases, plans))
        ns = {p.nsplit for p in plans}
        assert any(1 < v < 8 for v in ns) and any(v % 8 == 0 for v in ns) and any(v > 8 and v % 8 for v in ns), sorted(ns)
    bases = {W.expected_plan(c).base for c in W.CASES if c.regime == "one-split"}
    assert any(128 < v <= 256 for v in bases) and any(v > 256 for v in bases), "256 / base == 1, and == 0 clamped to one split"
    gauss = [c for c in W.CASES if c.name in W.GAUSSIAN]
    assert all({c.regime for c in gauss if c.dtype == dtype} == set(W.REGIMES) for dtype in ("bf16", "fp32")) and {W.expected_plan(c).variant for c in gauss} == {0, 1, 2, 3}
    assert all({c.dtype for c in gauss if c.name == name} == {"bf16", "fp32"} for name in W.GAUSSIAN)


def test_second_step_tile_lies_inside_the_output_grid():
    for case in W.CASES:
        n, od, oh, ow = W.second_step_tile(case)
        _, _, out, _ = W.geometry(case)
        assert 0 <= n < case.n and 0 <= od < out[0] and 0 <= oh < out[1] and 0 <= ow < out[2], case


def test_planner_rejections():
    """What gm_conv_wgrad_workspace_bytes refuses (-1) beyond test_native_planners_accept_and_reject_geometries_without_a_gpu."""
    ok = W.BY_ID["bf16-e3d-3x5x33"]
    flat = W.BY_ID["bf16-flat-volume-255"]
    assert _bytes(ok) > 0 and _bytes(flat) > 0
    # 2^31 voxels or more on either operand (the kernel's voxel index is 32-bit)
    assert _bytes(ok, N=1, Ds=1 << 11, Hs=1 << 10, Ws=1 << 10, Do=8, Ho=8, Wo=8) == -1
    assert _bytes(ok, N=1, Ds=8, Hs=8, Ws=8, Do=1 << 11, Ho=1 << 10, Wo=1 << 10) == -1
    assert _bytes(ok, N=1 << 16, Ds=32, Hs=32, Ws=32, Do=1, Ho=1, Wo=1) == -1            # N counts
    assert _bytes(ok, N=1, Ds=(1 << 11) - 1, Hs=1 << 10, Ws=1 << 10, Do=8, Ho=8, Wo=8) > 0  # one plane below the limit is planned
    # a depth stencil over a 1 x 1 plane stencil has no kernel
    assert _bytes(ok, kd=3, kh=1, kw=1) == -1
    assert _bytes(ok, kd=1, kh=3, kw=1) == -1 and _bytes(ok, kd=1, kh=1, kw=3) == -1
    # flat mode: stride 1, no padding
    assert _bytes(flat, stride=2) == -1
    for axis in ("pd", "ph", "pw"):
        assert _bytes(flat, **{axis: 1}) == -1
    # 16-byte loads: pointers and pitches
    for dtype, vec in (("bf16", 8), ("fp32", 4)):
        c = W.BY_ID[f"{dtype}-e3d-3x5x33"]
        assert _bytes(c) > 0
        assert _bytes(c, x=0x1008) == -1 and _bytes(c, gy=0x2004) == -1 and _bytes(c, x=0x1002) == -1
        assert _bytes(c, x_ld=c.cin + vec + 1) == -1 and _bytes(c, gy_ld=c.cout + vec // 2) == -1
        assert _bytes(c, x_ld=c.cin + 3 * vec, gy_ld=c.cout) > 0
    assert _bytes(ok, dtype=2) == -1
