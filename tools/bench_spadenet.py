"""Measures SPADENet on the MI355X (needs the GPU: fails without one).

    python tools/bench_spadenet.py [--seconds 1.0] [--out FILE]

Configuration: the reference's own test network (num_channels=[16, 32, 64, 128], z_dim=16, label_nc=3) at 2-D 4 x 1 x 256 x 256 and 3-D
1 x 1 x 64 x 64 x 64, fp32 and bf16.  Reports
  * the forward time per call (host clock around calls that end in a device synchronise, windows of at least --seconds after a warm-up),
  * the fused up = 1 dual-output spade_block_apply against the sequence it replaces on the same tensors, for the widest 3-D
    block that reads through an up-sampling (64 channels, 4^3 -> 8^3), the largest 3-D one (16 channels, 16^3 -> 32^3) and the largest 2-D one (16 channels,
    batch 4, 64^2 -> 128^2): resample2x + statistics pass + two single-output applies, built from ops that predate the fused kernel; the two alternate in
    one run,
  * the kernel's achieved bytes / s from shape-computed traffic (x once on the source grid, four maps and two outputs on the output grid) as a share of
    the 8.0 TB/s HBM3E peak (6.29 TB/s is what a float4 copy reaches).
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
NET = dict(in_channels=1, out_channels=1, label_nc=3, num_channels=[16, 32, 64, 128], z_dim=16)
SHAPES = {"2d": (4, (256, 256)), "3d": (1, (64, 64, 64))}


def _window(fn, seconds):
    """-> seconds per call over a window of at least `seconds` (device-synchronised at both ends)."""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        calls += 5
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / calls


def forward_times(seconds):
    from generativemodels_amd.networks.nets import SPADENet
    rows = []
    for tag, (n, sp) in SHAPES.items():
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(0)
            m = SPADENet(spatial_dims=len(sp), input_shape=list(sp), **{**NET, "num_channels": list(NET["num_channels"])}).eval().to("cuda", dtype)
            x = torch.randn((n, 1, *sp), device="cuda", dtype=dtype)
            seg = torch.nn.functional.one_hot(torch.randint(0, 3, (n, *sp), device="cuda"), 3).movedim(-1, 1).to(dtype).contiguous()
            with torch.no_grad():
                for _ in range(3):
                    m(seg, x)
                t = _window(lambda: m(seg, x), seconds)
                z = m.encode(x)
                td = _window(lambda: m.decode(seg, z), seconds)
            rows.append(dict(what="forward", shape=tag, batch=n, dtype=str(dtype).split(".")[-1], ms_per_forward=t * 1e3, ms_per_decode=td * 1e3))
            print(json.dumps(rows[-1]), flush=True)
            del m
    return rows


def fused_vs_composed(seconds, c, src, dtype, n=1):
    """One learned-shortcut block's norm_0 / norm_s pass behind an up-sampling: the fused kernel against resample2x + statistics + two applies."""
    from generativemodels_amd import ops
    osp = tuple(s * 2 for s in src)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((n, *src, c), device="cuda", generator=g).to(dtype)
    gb0 = torch.randn((n, *osp, 2 * c), device="cuda", generator=g).to(dtype)
    gb1 = torch.randn((n, *osp, 2 * c), device="cuda", generator=g).to(dtype)
    m0, m1 = (gb0[..., :c], gb0[..., c:]), (gb1[..., :c], gb1[..., c:])
    y0, y1 = (torch.empty((n, *osp, c), device="cuda", dtype=dtype) for _ in range(2))
    with torch.no_grad():
        scale, shift = ops.gn_scale_shift_composed(x, c, 1e-5, None, None)  # in the network: from the producing convolution's epilogue
        scale, shift = scale.clone(), shift.clone()

        def fused():
            ops.spade_block_apply(x, scale, shift, m0, m1, "leakyrelu", 0.2, True, out0=y0, out1=y1)

        def composed():
            xu = ops.resample2x(x, "up")
            sc, sh = ops.gn_scale_shift_composed(xu, c, 1e-5, None, None)
            h = ops.spade_apply(xu, sc, sh, m0[0], m0[1], "none", out=y0)
            ops.leaky_relu(h, 0.2)  # (gm_spade_apply has no LeakyReLU: without the new kernels this activation had no slope-0.2 form at all)
            ops.spade_apply(xu, sc, sh, m1[0], m1[1], "none", out=y1)

        def composed_without_activation():
            xu = ops.resample2x(x, "up")
            sc, sh = ops.gn_scale_shift_composed(xu, c, 1e-5, None, None)
            ops.spade_apply(xu, sc, sh, m0[0], m0[1], "none", out=y0)
            ops.spade_apply(xu, sc, sh, m1[0], m1[1], "none", out=y1)

        for f in (fused, composed, composed_without_activation):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        rounds = {"fused": [], "composed": [], "composed_without_activation": []}
        for _ in range(3):  # alternate: the machine is shared
            rounds["fused"].append(_window(fused, seconds / 3))
            rounds["composed"].append(_window(composed, seconds / 3))
            rounds["composed_without_activation"].append(_window(composed_without_activation, seconds / 3))
    es = x.element_size()
    vo, vs = n * int(torch.tensor(osp).prod()), n * int(torch.tensor(src).prod())
    traffic = es * c * (vs + 6 * vo)  # x on the source grid; (g0, b0, g1, b1) read and (y0, y1) written on the output grid
    best = {k: min(v) for k, v in rounds.items()}
    row = dict(what="fused_vs_composed", batch=n, channels=c, source=list(src), dtype=str(dtype).split(".")[-1],
               us={k: [round(t * 1e6, 2) for t in v] for k, v in rounds.items()}, best_us={k: round(t * 1e6, 2) for k, t in best.items()},
               fused_traffic_bytes=traffic, fused_bytes_per_s=traffic / best["fused"], fused_share_of_hbm_peak=traffic / best["fused"] / HBM_PEAK,
               fused_beats_composed=best["fused"] < best["composed_without_activation"],
               note="host-clock times of back-to-back calls (launch overhead included); kernel times: rocprofv3 --kernel-trace --stats")
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-forward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_spadenet.py needs the MI355X: no GPU found (nothing is measured on the CPU)")
    rows = [] if args.skip_forward else forward_times(args.seconds)
    for dtype in (torch.float32, torch.bfloat16):
        rows.append(fused_vs_composed(args.seconds, 64, (4, 4, 4), dtype))  # the widest 3-D block that reads through an up-sampling (64 -> 32 at 8^3)
        rows.append(fused_vs_composed(args.seconds, 16, (16, 16, 16), dtype))  # ... the largest 3-D one (16 -> 1 at 32^3)
        rows.append(fused_vs_composed(args.seconds, 16, (64, 64), dtype, n=4))  # ... and the largest 2-D one (16 -> 1 at 128^2, batch 4)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
