"""Times ops.resize / ops.resize_backward (gm_resize_taps, csrc/resize.hip) on one MI355X at conditioning-sized tensors.

Per shape, dtype and direction: `--window` seconds of back-to-back calls after a warm-up, timed twice over -- device events around the whole window
(time per call as the device saw it: the launches queue up, so this is kernel time plus whatever gap the host leaves) and the host clock around the
same window ending in a device synchronise.  Bytes are the compulsory traffic the op reports to the profiler (input + output + tables), so GB/s is
an EFFECTIVE rate over that call time, not a counter reading.  One JSON line per row on stdout and in --out.

    python tools/bench_resize.py --out profiles/resize_bench.jsonl"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generativemodels_amd import ops  # noqa: E402

# (label, mode, (N, *spatial, C), size, scale_factor)
SHAPES = [
    ("3-D mask to the latent grid, 1 ch", "trilinear", (1, 128, 128, 128, 1), None, 0.5),
    ("3-D mask to the latent grid, 1 ch", "area", (1, 128, 128, 128, 1), None, 0.5),
    ("3-D conditioning volume, 4 ch", "nearest", (1, 128, 128, 128, 4), (64, 64, 64), None),
    ("2-D images, 3 ch", "bilinear", (8, 512, 512, 3), None, 0.5),
    ("3-D features up, 8 ch", "trilinear", (1, 64, 64, 64, 8), None, 2.0),
    ("2-D features up, 16 ch", "bicubic", (4, 256, 256, 16), None, 2.0),
]


def _time(fn, window):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    reps = max(20, int(window / max((time.perf_counter() - t0) / 20, 1e-7)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / reps
    return reps, e0.elapsed_time(e1) * 1e-3 / reps, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    rows = []
    for label, mode, shape, size, sf in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            x = (torch.rand(shape, device="cuda") * 2 - 1).to(dtype)
            plan = ops.resize_plan(x, mode, size, sf)
            y = ops.resize(x, mode, plan=plan)
            for direction, src, fn in (("forward", x, lambda: ops.resize(x, mode, plan=plan)), ("gradient", y, lambda: ops.resize_backward(y, plan))):
                transposed = direction == "gradient"
                out_numel = x.numel() if transposed else y.numel()
                nbytes = (x.numel() + y.numel()) * x.element_size() + plan.table_bytes(transposed)
                reps, dev, host = _time(fn, args.window)
                row = dict(label=label, mode=mode, shape=list(shape), out_spatial=list(plan.out_spatial), dtype=str(dtype).split(".")[-1], direction=direction,
                           taps=plan.max_taps_transposed if transposed else plan.max_taps, vector_path=shape[-1] % (16 // x.element_size()) == 0,
                           outputs=out_numel, bytes=nbytes, reps=reps, device_us_per_call=round(dev * 1e6, 2), host_us_per_call=round(host * 1e6, 2),
                           effective_GBps_device=round(nbytes / dev / 1e9, 1))
                print(json.dumps(row), flush=True)
                rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
