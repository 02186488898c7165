"""CPU (-m "not gpu"): which of its three kernels the row GEMM takes (gm_rows_gemm_route, the function gm_rows_gemm itself switches on) pinned over
plain, affine and statistics-table descriptors, and the descriptors it refuses.  Descriptors carry dummy, 16-byte aligned, non-null pointers: the
route launches nothing and reads no operand.

The expected routes are derived by hand from the predicates of csrc/rows_gemm.hip, BK = 16 (fp32) / 32 (bf16), elt = 4 / 2 bytes:
  K-split: ceil(cin / BK) >= 8, rows <= 16, cin <= 1024 (fp32) / 2048 (bf16), rows * cin * elt <= 48 KiB -- and no (scale, shift) tables;
  else wide: statistic tables, or rows >= the gm_token_gemm_set_wide threshold (default 2048, 0 = never); cin % BK == 0; cout padded to 16 >= 32;
  else one 16-channel block per wave; statistic tables outside the wide kernel's geometry are an error."""
import ctypes as C
import os
import re

import pytest

from generativemodels_amd import _native
from generativemodels_amd._native import GmGnTables, GmRowsDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1  # GM_F32, GM_BF16
PTR = 0x10000     # dummy operand address (16-byte aligned, never read)
K = {k: int(v) for k, v in re.findall(r"#define (GM_ROWS_ROUTE_[A-Z]+) (\d+)", open(os.path.join(ROOT, "include", "gm_amd.h")).read())}
ROWS, KSPLIT, WIDE = K["GM_ROWS_ROUTE_ROWS"], K["GM_ROWS_ROUTE_KSPLIT"], K["GM_ROWS_ROUTE_WIDE"]
NAMES = {v: k for k, v in K.items()}


def desc(rows, cin, cout, dtype, affine=False, rows_per_sample=0, **fields):
    d = GmRowsDesc()
    d.x, d.w, d.y, d.x_ld, d.y_ld = PTR, PTR, PTR, cin, cout
    d.rows, d.cin, d.cout, d.dtype, d.rows_per_sample = rows, cin, cout, dtype, rows_per_sample
    if affine:
        d.pre_scale, d.pre_shift, d.ss_ld = PTR, PTR, cin
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def tables(cin, groups=32, rows=4):
    t = GmGnTables()
    t.stats[0], t.S[0], t.C[0], t.groups, t.eps = PTR, rows, cin, groups, 1e-5
    return t


def route(d):
    return _native.lib().gm_rows_gemm_route(C.byref(d))


class wide_from:
    """`with wide_from(min_rows, nb):` -- the process-wide threshold of the wide kernel, put back to its default on the way out."""

    def __init__(self, min_rows, nb=0):
        self.args = (min_rows, nb)

    def __enter__(self):
        _native.lib().gm_token_gemm_set_wide(*self.args)

    def __exit__(self, *exc):
        _native.lib().gm_token_gemm_set_wide(-1, 0)
        return False


def check(cases):
    got = [(what, NAMES.get(route(d), route(d))) for what, d, _ in cases]
    assert got == [(what, NAMES[want]) for what, _, want in cases]


def test_no_bench_switch_is_set():
    assert not [s for s in ("GM_LINEAR_KSPLIT", "GM_TOKEN_GEMM_WIDE", "GM_TOKEN_GEMM_WIDE_NB") if os.environ.get(s)]


def test_the_header_names_three_routes():
    assert sorted(K.values()) == [0, 1, 2] and len(K) == 3


def test_plain_rows_under_the_default_threshold():
    with wide_from(-1):
        check([("1x256->768 fp32", desc(1, 256, 768, F32), KSPLIT), ("1x256->768 bf16", desc(1, 256, 768, BF16), KSPLIT),
               ("5x64->257 fp32", desc(5, 64, 257, F32), ROWS), ("5x64->257 bf16", desc(5, 64, 257, BF16), ROWS),  # 4 / 2 K chunks
               ("17x1024->256 fp32", desc(17, 1024, 256, F32), ROWS), ("17x1024->256 bf16", desc(17, 1024, 256, BF16), ROWS),  # two row blocks
               ("12x2048->64 bf16", desc(12, 2048, 64, BF16), KSPLIT), ("12x1024->64 fp32", desc(12, 1024, 64, F32), KSPLIT),  # exactly 48 KiB
               ("13x1024->64 fp32", desc(13, 1024, 64, F32), ROWS), ("16x2048->64 bf16", desc(16, 2048, 64, BF16), ROWS),  # 52 / 64 KiB
               ("16x4096->64 bf16", desc(16, 4096, 64, BF16), ROWS)])  # beyond the staging pass's 2048 channels


def test_an_affine_prologue_never_takes_the_k_split_kernel():
    with wide_from(-1):
        check([("fp32", desc(8, 256, 256, F32, affine=True, rows_per_sample=8), ROWS),
               ("bf16", desc(8, 256, 256, BF16, affine=True, rows_per_sample=8), ROWS)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_affine_token_rows_around_the_wide_threshold(dtype):
    def tok(rows, cin, cout, rps=1024):
        return desc(rows, cin, cout, dtype, affine=True, rows_per_sample=rps)
    with wide_from(2048):
        check([("2048x64->192", tok(2048, 64, 192), WIDE), ("2047x64->192", tok(2047, 64, 192, rps=2047), ROWS),
               ("4096x80->192", tok(4096, 80, 192), WIDE if dtype == F32 else ROWS),  # 80 = 5 x 16, not a multiple of 32
               ("4096x64->16", tok(4096, 64, 16), ROWS), ("4096x64->17", tok(4096, 64, 17), WIDE)])  # padded cout 16 / 32
    with wide_from(0, 0):
        check([("never", tok(4096, 64, 192), ROWS)])
    with wide_from(1, 2):
        check([("always", tok(64, 64, 192, rps=64), WIDE)])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_statistic_tables_take_the_wide_kernel_under_every_threshold(dtype):
    t = tables(64)
    for threshold in (-1, 0, 1, 129, 2048):
        with wide_from(threshold):
            check([(f"threshold {threshold}", desc(128, 64, 192, dtype, rows_per_sample=64, gn=C.pointer(t), n_samples=2), WIDE)])


def test_refused_descriptors():
    lib = _native.lib()
    t80, t64 = tables(80, groups=5), tables(64)
    bad = [
        ("statistic tables with cin no multiple of BK", desc(128, 80, 192, BF16, rows_per_sample=64, gn=C.pointer(t80), n_samples=2), b"wide kernel"),
        ("V^T image in fp32", desc(128, 64, 192, F32, affine=True, rows_per_sample=64, vt=PTR, vt_c0=128, vt_dh=64), b"bf16"),
        ("V^T image with a residual", desc(128, 64, 192, BF16, affine=True, rows_per_sample=64, vt=PTR, vt_c0=128, vt_dh=64, res=PTR, res_ld=192), b"no residual"),
        ("scale without shift", desc(128, 64, 192, BF16, rows_per_sample=64, pre_scale=PTR, ss_ld=64), b"scale and shift come together"),
        ("rows_per_sample not dividing rows", desc(192, 64, 192, BF16, affine=True, rows_per_sample=128, vt=PTR, vt_c0=128, vt_dh=64), b"whole 64-key blocks"),
    ]
    with wide_from(-1):
        for what, d, names in bad:
            rc = route(d)
            assert rc < 0, (what, rc)
            assert names in lib.gm_last_error(), (what, lib.gm_last_error())
        # ... and each of them one field away from a descriptor the route accepts
        assert route(desc(128, 64, 192, BF16, rows_per_sample=64, gn=C.pointer(t64), n_samples=2)) == WIDE
        assert route(desc(128, 64, 192, BF16, affine=True, rows_per_sample=64, vt=PTR, vt_c0=128, vt_dh=64)) == ROWS
