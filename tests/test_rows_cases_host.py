"""CPU (-m "not gpu"): the row GEMM matrix of _rows_cases.py before it reaches a GPU (test_gpu_rows_matrix.py launches it).  Every case takes the kernel it
names (gm_rows_gemm_route on a dummy-pointer descriptor with the case's pitches); the routes, dtypes, tiers, activations and the geometric edges the matrix
is there for all occur; the exact tier is exact in fp32 in any summation order and blind to no K vector; the three misalignments of x are refused."""
import ctypes as C
import dataclasses

import torch

import _rows_cases as M
from _rows_cases import BF16, BK, CASES, DTYPES, F32, KSPLIT, ROWS, VECW, WIDE
from generativemodels_amd import _native
from test_rows_routes import PTR, route, wide_from


def _route(case, **kw):
    d, keep = M.describe(case, **kw)  # noqa: F841 -- keep: the tables d.gn points to
    with wide_from(1, case.nb) if case.route == WIDE else wide_from(-1):
        return route(d)


def test_the_case_count_is_within_the_cap():
    assert len(CASES) <= M.MAX_CASES
    assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
    count = {(M.ROUTE_NAME[r], M.NAME[dt]): sum(c.route == r and c.dtype == dt for c in CASES) for r in (ROWS, KSPLIT, WIDE) for dt in DTYPES}
    print(len(CASES), count)


def test_every_case_takes_the_kernel_it_names():
    got = [(c.id, M.route_name(_route(c))) for c in CASES]
    assert got == [(c.id, M.route_name(c.route)) for c in CASES]
    # ... and the (scale, shift) form of a statistics-form case, which the GPU test compares it with bit for bit
    assert all(_route(c, affine=True) == WIDE for c in M.GN_CASES)


def test_routes_dtypes_tiers_and_activations_all_occur():
    have = {(c.route, c.dtype, c.tier) for c in CASES}
    assert have == {(r, dt, t) for r in (ROWS, KSPLIT, WIDE) for dt in DTYPES for t in ("exact", "real")}
    real = {(c.route, c.dtype, c.post_act) for c in CASES if c.tier == "real"}
    assert real == {(r, dt, p) for r in (ROWS, KSPLIT, WIDE) for dt in DTYPES for p in M.POST_ACT}
    assert {c.pre_act for c in CASES if c.tier == "real"} == set(M.PRE_ACT)
    assert {(c.pre_act, c.post_act) for c in CASES if c.tier == "exact"} <= {(a, b) for a in ("none", "relu") for b in ("none", "relu")}
    for r in (ROWS, KSPLIT, WIDE):
        for dt in DTYPES:
            mine = [c for c in CASES if c.route == r and c.dtype == dt]
            assert {c.place for c in mine} == set(M.PLACES) and {c.xpad for c in mine} == {2, 3}
            assert {(c.bias, c.res) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(not c.affine for c in CASES if c.route == KSPLIT)


def test_the_geometric_edges_of_the_matrix_occur():
    for dt in DTYPES:
        bk, vw = BK[dt], VECW[dt]
        ex = [c for c in CASES if c.dtype == dt and c.tier == "exact"]
        rows_, ks, wide = ([c for c in ex if c.route == r] for r in (ROWS, KSPLIT, WIDE))
        assert {vw, bk - vw, bk, bk + vw, 4 * bk, 5 * bk, 7 * bk + vw, 1024} <= {c.cin for c in rows_}
        assert {1, 15, 16, 17, 33, 100} <= {c.rows for c in rows_} and {1, 15, 16, 17, 63, 64, 65, 257} <= {c.cout for c in rows_}
        assert any(c.affine and c.rows == 8 and c.cin == 8 * bk for c in rows_)
        assert any(c.rows == 16 and c.cin == (4096 if dt == BF16 else 2048) for c in rows_)
        assert any(c.affine and c.rps == 50 and c.rows == 150 for c in rows_) and any(c.affine and c.rps == 50 and c.rows == 150 for c in wide)
        chunks = lambda c: -(-c.cin // bk)
        for staged in (False, True):
            mine = [c for c in ks if (c.pre_act != "none") == staged]
            assert {8, 9, 15, 16, 17, 33, 64} <= {chunks(c) for c in mine}
            assert {8 * bk + vw, 16 * bk - vw} <= {c.cin for c in mine}
        assert {1, 2, 15, 16} <= {c.rows for c in ks} and {1, 16, 17, 100} <= {c.cout for c in ks}
        assert any(c.pre_act != "none" and c.rows * c.cin * (4 if dt == F32 else 2) == 48 * 1024 for c in ks)
        assert {(c.nb, c.cout) for c in wide} >= {(nb, co) for nb in (2, 3, 4) for co in (17, 30, 32, 36, 48, 80)}
        assert {5, 16, 63, 64, 65, 130} <= {c.rows for c in wide} and {bk, 2 * bk, 3 * bk, 5 * bk} <= {c.cin for c in wide}
        assert {c.place for c in wide if c.res and c.cout % 4 == 0} == set(M.PLACES)
        gn = [c for c in M.GN_CASES if c.dtype == dt]
        assert {(c.n_samples, c.cin, c.gn[0], c.gn[1]) for c in gn} == {(n, k, s, t) for n in (1, 2) for k in (2 * bk, 4 * bk) for s in (1, 2) for t in (1, 3)}
        assert all(c.rps == 64 for c in gn)
    vt = [c for c in CASES if c.vt]
    assert all(c.dtype == BF16 and c.tier == "exact" for c in vt)
    assert {(c.route, c.rps) for c in vt} == {(ROWS, 64), (ROWS, 128), (WIDE, 64)}
    assert any(c.vt[0] % 16 for c in vt) and any(c.vt[0] % 4 for c in vt) and any((c.cout - c.vt[0]) // c.vt[1] > 1 for c in vt)


def test_every_exact_geometry_occurs_without_an_output_activation():
    exact = [c for c in CASES if c.tier == "exact"]
    assert {c.geometry for c in exact} == {c.geometry for c in exact if c.post_act == "none"}


def test_exact_cases_are_exact_in_fp32_and_blind_to_no_k_vector():
    bad = []
    for c in CASES:
        if c.tier != "exact":
            continue
        o = M.operands(c)
        for name in ("x", "w", "res", "pro"):  # as the kernel holds them: in the case's dtype -- the prologue's output is re-packed to it
            t = o[name]
            assert t is None or torch.equal(t.to(c.dtype).double(), t), (c.id, name)
        assert torch.equal(o["pro"].to(BF16).double(), o["pro"]), c.id
        for name in ("bias", "scale", "shift"):
            t = o[name]
            assert t is None or torch.equal(t.float().double(), t), (c.id, name)
        # every value a multiple of 0.5, and the sum of the magnitudes of a row's terms below 2^23: every partial sum, in any order, is exact in fp32
        assert torch.equal((2 * o["pro"]).round(), 2 * o["pro"]) and torch.equal(o["w"].round(), o["w"]), c.id
        mass = o["pro"].abs() @ o["w"].abs().t() + 16
        assert mass.max().item() < 2 ** 23 and o["want"].abs().max().item() < 2 ** 24, c.id
        if c.post_act == "none":
            n = M.blind_pairs(c)
            if n:
                bad.append((c.id, n))
    assert not bad, bad


def test_the_blindness_count_sees_a_weightless_k_vector():
    """blind_pairs on doctored operands: K vector 1 of row 3 made weightless (its removal and its second count change nothing) is reported, twice."""
    c = next(c for c in CASES if c.tier == "exact" and c.post_act == "none" and c.affine and c.rows > 3 and c.cin >= 3 * VECW[c.dtype])
    o, vw = dict(M.operands(c)), VECW[c.dtype]
    assert M.blind_pairs(c, o) == 0
    o["pro"] = o["pro"].clone()
    o["pro"][3, vw:2 * vw] = 0
    o["want"] = M.epilogue(c, o, o["pro"] @ o["w"].t())
    assert M.blind_pairs(c, o) == 2


def test_the_statistics_form_reference_is_a_groupnorm():
    c = M.GN_CASES[0]
    o = M.operands(c)
    x = o["x"].reshape(c.n_samples, c.rps, M.GN_GROUPS, c.cin // M.GN_GROUPS)
    mean, var = x.mean((1, 3), keepdim=True), x.var((1, 3), unbiased=False, keepdim=True)
    want = ((x - mean) / (var + M.GN_EPS).sqrt()).reshape(c.rows, c.cin) * o["gamma"] + o["beta"]
    assert (M.PRE_FN[c.pre_act](want) - o["pro"]).abs().max().item() < 1e-12


def test_the_documented_v_image_permutation():
    keys = torch.arange(128)
    pos = M.vt_position(keys)
    assert sorted(pos.tolist()) == keys.tolist()
    blk, half, qq, r = keys // 32, (keys // 16) % 2, (keys // 4) % 4, keys % 4
    assert torch.equal(pos, blk * 32 + qq * 8 + half * 4 + r)


def test_misaligned_x_rows_are_refused():
    lib = _native.lib()
    for dt in DTYPES:
        es, vw = (4 if dt == F32 else 2), VECW[dt]
        for c in (next(c for c in CASES if c.dtype == dt and c.route == r and not c.gn) for r in (ROWS, KSPLIT, WIDE)):
            assert _route(c) == c.route
            one_off = []
            d, _ = M.describe(c, x=PTR + es)  # x offset by one element
            one_off.append(("x", d))
            d, _ = M.describe(c)
            d.x_ld += 1  # a pitch that is no multiple of the vector
            one_off.append(("x_ld", d))
            d, _ = M.describe(dataclasses.replace(c, cin=c.cin + vw // 2))
            d.x_ld = M.pitch(c, "x") + vw  # (a whole number of vectors, wide enough)
            one_off.append(("cin", d))
            with wide_from(1, c.nb) if c.route == WIDE else wide_from(-1):
                for what, d in one_off:
                    rc = lib.gm_rows_gemm_route(C.byref(d))
                    assert rc < 0, (c.id, what, rc)
                    assert b"x rows must be 16-byte vectors" in lib.gm_last_error(), (c.id, what, lib.gm_last_error())
