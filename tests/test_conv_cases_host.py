"""CPU (-m "not gpu"): the convolution forward matrix of _conv_cases.py before it reaches a GPU (test_gpu_conv_matrix.py launches it).  Every case, driven through
ops.conv on its placed CPU operands under _util.conv_on_cpu(), records the entry points and the cfg / ksplit of the GmConvDesc its route names; the families,
dtypes and tiers all occur; the exact tier keeps every value a kernel may round an integer of magnitude <= 256; on the reference alone, no (tap, 16-byte
channel vector) of any exact case is blind in any output-channel block of 16 and tile region it reaches, and each deliberate fault of the reference (the
mutants below) changes the expected output or statistics of an exact case on every family it can apply to.  No kernel is broken on purpose anywhere."""
import contextlib
import ctypes as C
import dataclasses
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _conv_cases as M
from _conv_cases import BF16, BK, CASES, DTYPES, F32, FAMILIES, VECW
from _util import conv_on_cpu
from generativemodels_amd import _native

EXACT = [c for c in CASES if c.tier == "exact"]
ENTRY_TAG = {"gm_gn_apply": "gn_apply", "gm_rows_gemm": "rows_gemm", "gm_copy_channels": "copy_channels"}
# entry points ops.start_profile() does not label: weight packing, the finalisation of a GroupNorm
QUIET = ("gm_pack_conv_weight", "gm_pack_subpixel_weight", "gm_gn_finalize_channels")


@contextlib.contextmanager
def switches(case):
    """The module switches of ops a case pins (COUT1_MARCH_LTD, ...), put back on exit."""
    from generativemodels_amd import ops
    todo = dict(case.switches)
    if case.ltd is not None:
        todo["COUT1_MARCH_LTD"] = case.ltd
    keep = {a: getattr(ops, a) for a in todo}
    try:
        for a, v in todo.items():
            setattr(ops, a, v)
        yield
    finally:
        for a, v in keep.items():
            setattr(ops, a, v)


def cpu_recipe(case):
    """A pending GroupNorm over empty statistic tables of 4 rows per part: enough for the plan, which reads no operand."""
    from generativemodels_amd import ops
    cs = [case.cin] if not case.split else [case.split, case.cin - case.split]
    stats = [torch.empty((4, case.n, c, 2), dtype=torch.float64) for c in cs]
    return ops.GnRecipe(stats, cs, case.n, 1, M.GN_GROUPS, M.GN_EPS, torch.ones(case.cin), torch.zeros(case.cin), stats[0].device)


@functools.lru_cache(maxsize=None)
def recorded(case):
    """-> (launch tags, the field dicts of the recorded GmConvDesc in order) of the case on CPU tensors."""
    from generativemodels_amd import ops
    fields = [f for f, _ in _native.GmConvDesc._fields_]
    o = M.operands(case)
    with conv_on_cpu() as rec, torch.no_grad(), switches(case):
        xs, w, bias, kw, _ = M.place(case, o, "cpu", recipe=cpu_recipe(case) if case.pre == "recipe" else None)
        rec.calls.clear()
        ops.conv(xs[0] if len(xs) == 1 else ops.VirtualCat(xs), w, bias, **kw)
        calls = list(rec.calls)
    tags, descs = [], []
    for row in calls:
        if row[0] == "gm_conv_forward":
            d = dict(zip(fields, row[1]))
            descs.append(d)
            tags.append(f"cfg{d['cfg']}{'k' if d['ksplit'] > 1 else ''}")
        elif row[0] not in QUIET:
            tags.append(ENTRY_TAG.get(row[0], row[0]))
    return tuple(tags), descs


def test_the_case_count_is_within_the_cap_and_every_cell_is_filled():
    assert len(CASES) <= M.MAX_CASES < 1000
    assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
    count = {}
    for c in CASES:
        key = (c.family, M.NAME[c.dtype], c.tier)
        count[key] = count.get(key, 0) + 1
    print(f"{len(CASES)} cases")
    for fam in FAMILIES:
        print("%-15s" % fam + "  ".join(f"{M.NAME[dt]} {t} {count.get((fam, M.NAME[dt], t), 0):3d}" for dt in DTYPES for t in ("exact", "real")))
    fallbacks = ("two_pass", "shortcut_first")  # host-side plans in front of kernels the matrix covers: exact tier only
    empty = [(fam, M.NAME[dt], t) for fam in FAMILIES for dt in DTYPES for t in ("exact", "real") if not count.get((fam, M.NAME[dt], t))
             and not (fam in fallbacks and t == "real")]
    assert not empty, empty


def test_every_case_takes_the_route_it_names():
    bad = []
    for c in CASES:
        try:
            tags, descs = recorded(c)
        except Exception as ex:  # noqa: BLE001 -- a refused case is listed with the others
            bad.append((c.id, f"{type(ex).__name__}: {ex}"))
            continue
        if tags != c.route:
            bad.append((c.id, tags))
            continue
        d = descs[-1]
        if c.slices != (d["ksplit"] if d["ksplit"] > 1 else 0):
            bad.append((c.id, f"ksplit {d['ksplit']}"))
        if c.cfg is not None and d["cfg"] != c.cfg:
            bad.append((c.id, f"cfg {d['cfg']}"))
        if c.recipe_at is not None:  # the statistic tables in the descriptor of the kernel the plan names: cfg 24 / 25 unsplit, or the K slices of cfg 11
            at = None if not (d["pre_stats"][0] and not d["pre_scale"]) else ("slices" if d["cfg"] == 11 and d["ksplit"] > 1 else
                                                                                ("descriptor" if d["cfg"] in (24, 25) and d["ksplit"] <= 1 else "?"))
            parts = [bool(p) for p in d["pre_stats"]], list(d["pre_C"]), list(d["pre_S"])
            want_parts = ([True, bool(c.split)], [c.split or c.cin, c.cin - c.split if c.split else 0], [4, 4 if c.split else 0])
            if at != c.recipe_at or parts != want_parts or d["pre_groups"] != M.GN_GROUPS:
                bad.append((c.id, f"the recipe is finalised at {at}, tables {parts}"))
        if bool(d["x2"]) != bool(c.split and c.family != "two_pass") or bool(d["skip_x"][0]) != bool(c.skip and c.family != "shortcut_first"):
            bad.append((c.id, "second source / shortcut not where the family reads it"))
        # a slice at channel 3 or with a pitch that is no vector multiple takes the scalar epilogue: no fused statistics (gm_conv_stats_slots = 0) -- except
        # on cfg 24 / 25, which count whatever they store
        if c.stats and bool(d["stats"]) != (M.vector_epilogue(c) or c.family in ("sn3d", "sn2d")) and c.family not in ("generic",):
            bad.append((c.id, f"statistics pointer {d['stats']}"))
        if c.family == "generic" and d["stats"]:
            bad.append((c.id, "the generic kernels fuse no statistics"))
    assert not bad, f"{len(bad)} cases:\n" + "\n".join(f"{i}: {t}" for i, t in bad[:60])


def launch_tile(c):
    """-> (the recorded GmConvDesc of the case's last launch, its tile (d, h, w) from the descriptor's own tile bits, its channel block from gm_conv_cfg_tile)."""
    d = recorded(c)[1][-1]
    bm, bn = C.c_int(), C.c_int()
    assert _native.lib().gm_conv_cfg_tile(d["cfg"], C.byref(bm), C.byref(bn)) == 0
    return d, (1 << d["ltd"], 1 << d["lth"], 1 << d["ltw"]), bn.value


def work_groups(c):
    """Work-groups of the case's last launch, by the grid arithmetic of gm_conv_forward on the recorded descriptor: tiles x channel blocks (x K slices; the
    sub-pixel launch walks the low-resolution grid once per (d, h) parity; cfg 25 at stride 2 walks 2 n - 1 positions)."""
    d, (td, th, tw), bn = launch_tile(c)
    sub, walk2 = d["cfg"] == 17, d["cfg"] == 25 and d["sh"] == 2
    de, he, we = (d["Ds"], d["Hs"], d["Ws"]) if sub else (d["Do"], 2 * d["Ho"] - 1 if walk2 else d["Ho"], 2 * d["Wo"] - 1 if walk2 else d["Wo"])
    return d["N"] * -(-de // td) * -(-he // th) * -(-we // tw) * -(-d["Cout"] // bn) * (4 if sub else 1) * (d["ksplit"] if d["ksplit"] > 1 else 1)


def test_the_fast_variants_refuse_a_larger_patch():
    for dt in DTYPES:
        for c in (c for c in EXACT if c.dtype == dt and c.family == "fast" and c.k > 3):
            assert c.k == M.FAST_MAX_K[c.cfg] and recorded(c)[0] == c.route
            with pytest.raises(ValueError):
                recorded(dataclasses.replace(c, k=c.k + 2, pad=c.k // 2 + 1))


def test_the_fast_variants_refuse_a_volume_axis_of_extent_1():
    """In 3-D the tile bits an extent-1 axis cannot take go to W (ops._tile_bits_fast) and the patch outgrows gm_conv_fast_max_patch on every variant: the reason
    the matrix holds extent 2 but not extent 1 for this family's volumes."""
    for dt in DTYPES:
        for cfg in (5, 6, 7, 8, 9, 10):
            for sp in ((1, 16, 16), (16, 1, 16), (16, 16, 1)):
                with pytest.raises(ValueError):
                    recorded(M.Case("exact", "fast", (f"cfg{cfg}",), dt, 1, 2 * VECW[dt], 24, sp, cfg=cfg))


def test_families_edges_and_epilogues_all_occur():
    for dt in DTYPES:
        bk, vw = BK[dt], VECW[dt]
        ex = [c for c in EXACT if c.dtype == dt]
        fam = lambda f: [c for c in ex if c.family == f]
        assert {c.cfg for c in fam("generic")} == {0, 1, 2, 3, 4} and {c.cfg for c in fam("fast")} == {5, 6, 7, 8, 9, 10}
        assert {c.cfg for c in fam("dma")} == {11, 14, 16, 18, 19} and {c.cfg for c in fam("dma_s2")} == {15}
        gen = fam("generic")
        assert {1, 3, 4} <= {c.k for c in gen} and {1, 2, 3} == {c.nsp for c in gen} and any(c.stride == 2 for c in gen) and any(c.dil == 2 for c in gen)
        assert any(c.pad_hi is not None and c.pad_hi != c.pad for c in gen) and any(c.up for c in gen)
        assert {0, 1} <= {c.opad for c in gen if c.T and c.stride == 2} and {3, 5, vw + 1} <= {c.cin for c in gen}
        assert {15, 16, 17, 63, 64, 65, 136} <= {c.cout for c in gen}
        for cfg in (11, 14, 16, 18, 19, 24, 15):  # each axis of the family's own tile at one less / equal / one more; the other extents 1 and 2
            td, th, tw = M.TILE[cfg]
            mine = [c for c in ex if c.cfg == cfg]
            for ax, t in enumerate((td, th, tw)):
                assert {t - 1, t, t + 1} <= {c.osp[ax] for c in mine if c.nsp == 3}, (cfg, ax)
            assert {1, 2} <= {v for c in mine for v in c.osp} and {1, 2} <= {c.n for c in mine}
        sn2 = [c for c in fam("sn2d") if c.stride == 1 and not c.up]
        assert all({15, 16, 17} <= {c.osp[ax] for c in sn2} for ax in (0, 1)) and {1, 2} <= {v for c in sn2 for v in c.osp}
        s2 = [c for c in fam("sn2d") if c.stride == 2]
        assert {0, 1} <= {v % 2 for c in s2 for v in c.sp} and {0, 1} <= {v % 2 for c in s2 for v in c.osp}
        sub = fam("subpixel")
        assert any(c.up for c in sub) and {(3, 1), (4, 0)} <= {(c.k, c.opad) for c in sub if c.T}
        assert all({3, 4, 5} <= {c.sp[ax] for c in sub} for ax in (0, 1)) and {15, 16, 17} <= {c.sp[2] for c in sub}
        for f in ("sn3d", "sn2d"):
            assert {1, 4, 6, 15, 16, 17, 40} <= {c.cout for c in fam(f)} and {"none", "tables"} <= {c.pre for c in fam(f)}
            assert {c.place for c in fam(f)} == set(M.PLACES) | {"dense"}
            assert any(c.pre == "recipe" and c.recipe_at == "descriptor" for c in CASES if c.family == f and c.dtype == dt)
        for cfg in (8, 11, 14, 16, 18, 19, 24, 25, 15, 12, 13, 20):  # work-group counts around the 8-XCD remap
            assert {1, 7, 8, 9, 17} <= {work_groups(c) for c in ex if c.cfg == cfg and not c.slices}, cfg
        assert {8, 9} <= {work_groups(c) for c in fam("splitk")} and {4, 8} <= {work_groups(c) for c in fam("subpixel")}
        dma = fam("dma")
        assert {1, 2, 3, 6} <= {c.cin // bk for c in dma} and {2 * vw, 64 - vw, 64, 64 + vw, 136} <= {c.cout for c in dma}
        for cfg in (11, 14, 16, 18, 19):
            mine = [c for c in dma if c.cfg == cfg]
            assert any(c.split == bk for c in mine) and any(c.split and c.split % bk == 0 and 2 * c.split != c.cin and c.split > bk for c in mine)
            assert {1, 2} <= {len(c.skip) for c in mine if c.skip} and any(sum(c.skip) // bk > 2 for c in mine) and any(c.pre == "tables" for c in mine)
        s2 = fam("dma_s2")  # cfg 15 reads a second source and the fused shortcut like the stride-1 configurations
        assert any(c.split == bk for c in s2) and any(c.split > bk and 2 * c.split != c.cin for c in s2) and {1, 2} <= {len(c.skip) for c in s2 if c.skip}
        assert any(sum(c.skip) // bk > 2 for c in s2)
        for cfg in (5, 6, 7, 8, 9, 10):  # a volume axis of extent 2 on every fast variant (extent 1: test_the_fast_variants_refuse_a_volume_axis_of_extent_1)
            assert any(c.cfg == cfg and c.nsp == 3 and 2 in c.osp for c in fam("fast")), cfg
        assert all({1, 2} <= {c.sp[ax] for c in fam("march")} for ax in (1, 2)) and all({1, 2} <= {c.sp[ax] for c in fam("subpixel")} for ax in (0, 1, 2))
        wide = [c for c in fam("march") if dict(c.switches).get("COUT1_MARCH_LTW_128B") == 5]
        assert {31, 32, 33} <= {c.sp[2] for c in wide} and all(launch_tile(c)[1] == (4, 8, 32) for c in wide)
        sk = fam("splitk")
        assert {(3, 2), (12, 6), (9, 5)} <= {(c.cin // bk, c.slices) for c in sk} and {(12, 8), (9, 8)} <= {(c.cin // bk, c.ksplit) for c in sk}
        assert {2, 3, 4, 5, 6, 7, 8} <= {c.ksplit for c in sk}
        assert {15, 16, 17, 63, 64, 65, 136} <= {c.cout for c in fam("fast")}
        assert any(c.res for c in sk) and any(c.skip for c in sk) and all(c.stats for c in sk) and any(c.split for c in sk)
        assert any(c.pre == "recipe" and c.recipe_at == "slices" for c in CASES if c.family == "splitk" and c.dtype == dt)
        assert {1, 2, 3, 4} == {c.cin for c in fam("cin")} and {2, 3} == {c.nsp for c in fam("cin")}
        assert {c.cin // bk for c in fam("cout1")} == ({2, 4, 8} if dt == F32 else {2, 4})
        march = fam("march")
        assert {c.cin * (4 if dt == F32 else 2) for c in march} == {128, 256} and {2, 3, 4, 5} == {c.ltd for c in march}
        assert all({(1 << l), (1 << l) + 1} <= {c.sp[0] for c in march if c.ltd == l} for l in (2, 3, 4, 5)) and min(c.sp[0] for c in march) == 4
        assert {"copy_channels", "gn_apply"} <= {c.route[0] for c in fam("two_pass")} and all(c.split for c in fam("two_pass")) and all(c.skip for c in fam("shortcut_first"))
        for f in FAMILIES:  # a non-zero shift in front of every family that takes a prologue
            if f not in ("subpixel", "cin", "dma_s2", "shortcut_first"):
                assert any(c.pre == "tables" and float(M.operands(c)["shift"].abs().max()) > 0 for c in fam(f)), f
        real = {(c.family, c.post_act) for c in CASES if c.tier == "real" and c.dtype == dt}
        assert real >= {(f, p) for f in FAMILIES if f not in ("two_pass", "shortcut_first") for p in M.POST_ACT}
        assert any(c.pre_act == "silu" for c in CASES if c.tier == "real" and c.dtype == dt)
        for f in ("generic", "fast", "dma", "dma_s2", "splitk", "subpixel", "sn3d", "sn2d"):
            assert any(c.cin >= 16 * bk for c in CASES if c.tier == "real" and c.dtype == dt and c.family == f), f
    assert {(c.pre_act, c.post_act) for c in EXACT} <= {(a, b) for a in ("none", "relu") for b in ("none", "relu")}
    assert all(c.n * math.prod(c.osp) <= 9000 for c in CASES)  # (the 17-work-group launches of the 512-voxel tiles are the largest)


def test_the_two_forms_of_the_reference_agree():
    for c in CASES:
        o = M.operands(c)
        phi = c.pad if c.pad_hi is None else c.pad_hi
        if c.T and phi != c.pad:
            continue
        other = M.reference_torch(c, o)
        assert other.shape == o["want"].shape == (c.n, *c.osp, c.cout), c.id
        if c.tier == "exact":
            assert torch.equal(other, o["want"]), c.id
        else:
            assert (other - o["want"]).abs().max().item() <= 1e-11 * max(1.0, o["want"].abs().max().item()), c.id


def test_exact_cases_keep_every_rounding_point_an_integer_within_the_bound():
    worst = {}
    for c in EXACT:
        o = M.operands(c)
        for name in ("x", "w", "res", "bias", "rowvec", "scale", "shift", "skip_w", "skip_b"):
            t = o[name]
            assert t is None or torch.equal(t.round(), t), (c.id, name)
        assert float(o["w"].abs().min()) == 1.0 and (o["skip_w"] is None or float(o["skip_w"].abs().min()) == 1.0), c.id
        top = 0.0
        for t in M.rounding_points(c, o) + [o["want"]]:
            assert torch.equal(t.round(), t), c.id
            top = max(top, t.abs().max().item())
        assert top <= M.EXACT_BOUND, (c.id, top)
        assert torch.equal(M.rounded(o["want"], BF16).double(), o["want"]), c.id
        # the statistics: every partial sum of the stored values and of their squares, in any order, is an integer below 2^24 (exact in fp32)
        assert o["stats"].abs().max().item() < 2 ** 24 and (o["want"] ** 2).reshape(c.n, -1, c.cout).sum(1).max().item() < 2 ** 24, c.id
        worst[c.family] = max(worst.get(c.family, 0.0), top)
    print({k: int(v) for k, v in worst.items()})


# ---- sensitivity: what a single (tap, channel vector) weighs in the reference --------------------------------------------------------------------------
def region_tile(case):
    """The block of OUTPUT voxels one work-group of the case's last launch owns, (d, h, w), from the tile bits of the recorded descriptor: the sub-pixel tile
    walks the low-resolution grid (twice the extent of the output), cfg 25 at stride 2 the stride-1 grid (half of it)."""
    d, tile, _ = launch_tile(case)
    if d["cfg"] == 17:
        return tuple(2 * v for v in tile)
    if d["cfg"] == 25 and d["sh"] == 2:
        return (1, tile[1] // 2, tile[2] // 2)
    return tile


def blind_tuples(case, o=None, thin=1):
    """(tap, channel vector, block of 16 output channels, region) tuples of an exact case in which removing that slice of the weight
    changes NO rounded output although the tap reaches the region without padding -- plus the same for every 16-byte vector of shortcut channels.  One grouped
    convolution per case: group g = channel vector g, its outputs the (tap, Cout) pairs.  Counted on the value in front of the output activation (what the
    kernel accumulates: a ReLU behind it is the same code on every route).  thin: every thin-th vector only."""
    assert case.tier == "exact"
    o = M.operands(case) if o is None else o
    before = M.epilogue(dataclasses.replace(case, post_act="none"), o, M.accumulate(case, o))
    vw = VECW[case.dtype]
    e, m, w3, s3, d3 = M.effective(case, o)
    cout, cin = w3.shape[:2]
    taps = w3.shape[2] * w3.shape[3] * w3.shape[4]
    nv = -(-cin // vw)
    pad_c = nv * vw - cin
    e, w3 = F.pad(e, (0, 0) * 3 + (0, pad_c)), F.pad(w3, (0, 0) * 3 + (0, pad_c))
    vecs = list(range(0, nv, thin))
    sel = torch.tensor([v * vw + i for v in vecs for i in range(vw)])
    # weight of group v: [taps * cout, vw, kd, kh, kw], output (t, co) = the tap-t slice of w[co] over the vector's channels alone
    wv = w3[:, sel].reshape(cout, len(vecs), vw, taps).permute(1, 3, 0, 2)  # [v, t, co, i]
    wg = torch.zeros((len(vecs), taps, cout, vw, taps), dtype=torch.float64)
    wg[:, torch.arange(taps), :, :, torch.arange(taps)] = wv.permute(1, 0, 2, 3)
    wg = wg.reshape(len(vecs) * taps * cout, vw, *w3.shape[2:])
    contrib = F.conv3d(e[:, sel], wg, None, stride=s3, dilation=d3, groups=len(vecs))  # [N, v * t * co, Do, Ho, Wo]
    n, _, do, ho, wo = contrib.shape
    contrib = contrib.reshape(n, len(vecs), taps, cout, do, ho, wo)
    want = M._to3(before).reshape(n, 1, 1, cout, do, ho, wo)
    changed = (M.rounded(want - contrib, case.dtype) != M.rounded(want, case.dtype)).double()
    one_hot = torch.zeros((taps, 1, *w3.shape[2:]), dtype=torch.float64)
    one_hot.reshape(taps, taps)[torch.arange(taps), torch.arange(taps)] = 1.0
    reach = F.conv3d(m, one_hot, None, stride=s3, dilation=d3).expand(n, taps, do, ho, wo)  # 1 where the tap reads data

    def pooled(t, cblock):  # max over regions (and blocks of 16 channels at dim `cblock`)
        td, th, tw = region_tile(case)
        lead = t.shape[:-3]
        t = F.max_pool3d(t.reshape(-1, 1, do, ho, wo), (td, th, tw), ceil_mode=True).reshape(*lead, -1)
        if cblock is not None:
            t = t.movedim(cblock, -1)
            t = F.max_pool1d(t.reshape(-1, 1, cout), 16, ceil_mode=True).reshape(*t.shape[:-1], -1)
        return t
    seen = pooled(changed, 3)                        # [n, v, t, regions, blocks]
    reached = pooled(reach, None)[:, None, :, :, None]  # [n, 1, t, regions, 1]
    blind = int(((seen == 0) & (reached > 0)).sum())
    if case.skip and case.family != "shortcut_first":
        sx, sw = torch.cat(o["skip_x"], -1), o["skip_w"]
        sc = sx.shape[-1] // vw
        contrib = torch.einsum("...vi,cvi->...vc", sx.reshape(*sx.shape[:-1], sc, vw), sw.reshape(cout, sc, vw)).movedim(-2, 1)  # [N, v, *osp, Cout]
        full = before.unsqueeze(1)
        ch = (M.rounded(full - contrib, case.dtype) != M.rounded(full, case.dtype)).double()
        ch = M._to3(ch.reshape(n * sc, *case.osp, cout)).reshape(n, sc, cout, do, ho, wo)
        blind += int((pooled(ch, 2) == 0).sum())
    return blind


def test_no_tap_or_channel_vector_is_blind_in_any_exact_case():
    bad, counted = [], 0
    for c in EXACT:
        counted += 1
        b = blind_tuples(c)
        if b:
            bad.append((c.id, b))
    print(f"{counted} exact cases, blind tuples: {sum(b for _, b in bad)}")
    assert not bad, "\n".join(f"{b} {i}" for i, b in bad)
    assert counted == len(EXACT)


def test_the_blindness_count_sees_a_weightless_slice():
    """blind_tuples on doctored operands: with the input of channel vector 1 zeroed, every tap of that vector is reported in every block and region it reaches."""
    c = next(c for c in EXACT if c.post_act == "none" and c.family == "dma" and c.pre == "none" and not c.split and not c.skip and not c.up and c.cin >= 3 * VECW[c.dtype])
    o, vw = dict(M.operands(c)), VECW[c.dtype]
    assert blind_tuples(c, o) == 0
    o["x"] = o["x"].clone()
    o["x"][..., vw:2 * vw] = 0
    assert blind_tuples(c, o) >= 27


# ---- reference mutants -------------------------------------------------------------------------------------------------------------------------------------
def _stats_of(c, want):
    stored = M.rounded(want, c.dtype).double().reshape(c.n, -1, c.cout)
    return torch.stack([stored.sum(1), (stored * stored).sum(1)], -1)


def mutant_tap_dropped_on_a_face(c, o):
    """The first tap that reaches the last plane of the W axis is dropped there only."""
    e, m, w3, s3, d3 = M.effective(c, o)
    w1 = torch.zeros_like(w3)
    w1[:, :, 0, 0, 0] = w3[:, :, 0, 0, 0]
    part = M._from3(F.conv3d(e, w1, None, stride=s3, dilation=d3), c.nsp)
    part[..., :-1, :] = 0
    return M.epilogue(c, o, M.accumulate(c, o) - part), None


def mutant_padding_holds_act_of_shift(c, o):
    if c.pre != "tables":
        return None
    return M.epilogue(c, o, M.accumulate(c, o, pad_value=M.PRE_FN[c.pre_act](o["shift"]))), None


def mutant_halo_of_sample_1_from_sample_0(c, o):
    if c.n < 2 or c.pad == 0 or c.T:
        return None
    return M.epilogue(c, o, M.accumulate(c, o, halo_from_previous=True)), None


def mutant_shortcut_bias_omitted(c, o):
    return M.epilogue(c, o, M.accumulate(c, o), skip_bias=False) if c.skip else None, None


def mutant_residual_after_activation(c, o):
    if not c.res or c.post_act == "none":
        return None
    return M.epilogue(c, o, M.accumulate(c, o), res_after_act=True), None


def mutant_statistics_over_the_padded_tile(c, o):
    """The voxels a tile holds beyond the volume counted too: each would store post_act(bias + row) (no input reaches it; the residual and shortcut read as 0)."""
    if not c.stats or c.family in ("generic", "two_pass", "shortcut_first") or not (M.vector_epilogue(c) or c.family in ("sn3d", "sn2d")):
        return None
    td, th, tw = region_tile(c)
    o3 = (1,) * (3 - c.nsp) + c.osp
    extra = (-(-o3[0] // td) * td) * (-(-o3[1] // th) * th) * (-(-o3[2] // tw) * tw) - o3[0] * o3[1] * o3[2]
    if not extra:
        return None
    v = torch.zeros((c.n, c.cout), dtype=torch.float64)
    if o["bias"] is not None:
        v = v + o["bias"]
    if o["rowvec"] is not None:
        v = v + o["rowvec"]
    if c.skip:
        v = v + o["skip_b"]
    v = M.POST_FN[c.post_act](v)
    return o["want"], o["stats"] + extra * torch.stack([v, v * v], -1)


def mutant_last_k_slice_twice(c, o):
    if not c.slices:
        return None
    lo, hi = M.slice_channels(c)
    keep = torch.zeros(c.cin, dtype=torch.float64)
    keep[lo:hi] = 1.0
    e, _, w3, s3, d3 = M.effective(c, o)
    part = M._from3(F.conv3d(e * keep.reshape(1, -1, 1, 1, 1), w3, None, stride=s3, dilation=d3), c.nsp)
    return M.epilogue(c, o, M.accumulate(c, o) + part), None


def mutant_stride_2_from_odd_positions(c, o):
    if not (c.family == "sn2d" and c.stride == 2):
        return None
    c1 = dataclasses.replace(c, stride=1)
    full = M.accumulate(c1, o)  # the stride-1 walk over the same padded image
    odd = full[:, 1::2, 1::2]
    acc = M.accumulate(c, o)
    if odd.shape != acc.shape:
        hh, ww = min(odd.shape[1], acc.shape[1]), min(odd.shape[2], acc.shape[2])
        acc2 = acc.clone()
        acc2[:, :hh, :ww] = odd[:, :hh, :ww]
        odd = acc2
    return M.epilogue(c, o, odd), None


def mutant_parity_images_swapped(c, o):
    if c.family != "subpixel":
        return None
    acc = M.accumulate(c, o).clone()
    even, odd = acc[..., 0::2, :].clone(), acc[..., 1::2, :].clone()
    acc[..., 0::2, :], acc[..., 1::2, :] = odd, even
    return M.epilogue(c, o, acc), None


MUTANTS = {  # name -> (the fault, the families it can apply to)
    "one tap dropped on one face only": (mutant_tap_dropped_on_a_face, FAMILIES),
    "padding left at act(shift) after a prologue": (mutant_padding_holds_act_of_shift, tuple(f for f in FAMILIES if f not in ("subpixel", "cin", "dma_s2", "shortcut_first"))),
    "the halo of sample 1 read from sample 0": (mutant_halo_of_sample_1_from_sample_0, FAMILIES),
    "the shortcut bias omitted": (mutant_shortcut_bias_omitted, ("dma", "dma_s2", "splitk", "sn3d", "sn2d", "shortcut_first")),
    "the residual added after the activation": (mutant_residual_after_activation, tuple(f for f in FAMILIES if f not in ("two_pass", "shortcut_first"))),
    "statistics over tile-padded voxels": (mutant_statistics_over_the_padded_tile, ("fast", "dma", "dma_s2", "splitk", "subpixel", "sn3d", "sn2d", "cin")),
    "the last K slice counted twice": (mutant_last_k_slice_twice, ("splitk",)),
    "stride-2 output from the odd positions of the stride-1 walk": (mutant_stride_2_from_odd_positions, ("sn2d",)),
    "a sub-pixel parity image swapped": (mutant_parity_images_swapped, ("subpixel",)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_reference_mutant_is_detected_on_every_family_it_applies_to(name):
    fault, families = MUTANTS[name]
    caught = {f: 0 for f in families}
    for c in EXACT:
        if c.family not in families:
            continue
        o = M.operands(c)
        got = fault(c, o)
        if got is None or got[0] is None:
            continue
        want, stats = got
        stats = _stats_of(c, want) if stats is None else stats
        if not torch.equal(M.rounded(want, c.dtype), M.rounded(o["want"], c.dtype)) or (c.stats and not torch.equal(stats, o["stats"])):
            caught[c.family] += 1
    print(name, caught)
    assert all(caught.values()), (name, caught)
