"""GPU: the bits and the native launches of the convolution layers' forward + backward, for comparing two trees of the Python package over ONE built library.
For a fixed seeded case list through the six public wrappers (autograd.conv / linear / conv_transpose / conv_dilated / conv_transpose_dilated / upsample_conv)
-- and autograd.silu, whose backward is the convolutions' activation backward -- it records per case the sha256 of y, dx, dW, db (drow, dres where present)
and the ordered names of the native calls (ops.check's `what`).
usage: python tools/conv_backward_digest.py [--tree DIR] --out FILE      (DIR holds the generativemodels_amd to import; GM_NATIVE_LIB names the library)
       python tools/conv_backward_digest.py --compare A.json B.json      (exit status 1 unless every digest and every call list is equal)"""
import argparse
import hashlib
import json
import os
import sys
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
args = ap.parse_args()

if args.compare:
    a, b = (json.load(open(p)) for p in args.compare)
    differ = [c for c in sorted(set(a) | set(b)) if a.get(c) != b.get(c)]
    for c in differ:
        ca, cb = a.get(c) or {}, b.get(c) or {}
        what = [k for k in sorted(set(ca.get("sha", {})) | set(cb.get("sha", {}))) if ca.get("sha", {}).get(k) != cb.get("sha", {}).get(k)]
        print(f"DIFFERS {c}: digests {what or 'equal'}; calls {'equal' if ca.get('calls') == cb.get('calls') else 'differ'}"
              + "".join(f"\n    {p}: {v['error']}" for p, v in zip(args.compare, (ca, cb)) if "error" in v))
    print(f"{len(a)} / {len(b)} cases, {len(set(a) | set(b)) - len(differ)} equal in every digest and call list, {len(differ)} differ; "
          f"{sum(len(v.get('calls', ())) for v in a.values())} / {sum(len(v.get('calls', ())) for v in b.values())} native calls")
    sys.exit(1 if differ or not a else 0)

sys.path.insert(0, os.path.abspath(args.tree))
import torch

import generativemodels_amd as gm
from generativemodels_amd import autograd as A
from generativemodels_amd import ops

assert os.path.dirname(os.path.abspath(gm.__file__)) == os.path.join(os.path.abspath(args.tree), "generativemodels_amd"), gm.__file__
DEV = "cuda"
CALLS = []
_check = ops.check


def _recording_check(rc, what=""):
    CALLS.append(what)
    return _check(rc, what)


ops.check = _recording_check  # (the launches of ops.py resolve `check` in their module at call time)
RESULTS = {}


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def randn(gen, shape, dtype, scale=1.0, grad=True):
    return (torch.randn(shape, generator=gen) * scale).to(DEV, dtype).requires_grad_(grad)


def case(name, dtype, fn, x_shape, w_shape, rowvec=None, res=None, wdtype=None, wrap=None, transposed=False):
    """fn(x, weight, bias, rowvec=, res=) -> y over seeded operands; rowvec: rows of the fp32 row vector; res: the residual's shape; transposed: the
    weight is [Cin, Cout, *k]."""
    name = f"{name} {str(dtype).split('.')[-1]}"
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    wdtype = wdtype or dtype
    cout = w_shape[1] if transposed else w_shape[0]
    t = dict(x=randn(gen, x_shape, dtype), weight=randn(gen, w_shape, wdtype, 0.1), bias=randn(gen, (cout,), wdtype))
    extra = {}
    if rowvec is not None:
        extra["rowvec"] = t["rowvec"] = randn(gen, (rowvec, cout), torch.float32)
    if res is not None:
        extra["res"] = t["res"] = randn(gen, res, dtype)
    del CALLS[:]
    try:
        run = (lambda: fn(t["x"], t["weight"], t["bias"], **extra))
        y = wrap(run) if wrap else run()
        y.backward((torch.randn(y.shape, generator=gen)).to(DEV, y.dtype))
        torch.cuda.synchronize()
        RESULTS[name] = dict(sha=dict(y=sha(y), **{"d" + k: sha(v.grad) for k, v in t.items()}), calls=list(CALLS))
    except Exception as e:  # a case that raises is recorded as such: the comparison shows it
        RESULTS[name] = dict(error=f"{type(e).__name__}: {e}", calls=list(CALLS))


def conv(**kw):
    return lambda x, w, b, **extra: A.conv(x, w, b, **kw, **extra)


for dt in (torch.float32, torch.bfloat16):
    k3 = (3, 3, 3)
    case("conv k3 s1 p1 rowvec res", dt, conv(kernel=3, padding=1), (2, 8, 8, 8, 32), (32, 32, *k3), rowvec=2, res=(2, 8, 8, 8, 32))
    case("conv k3 s1 p1 one-row rowvec res", dt, conv(kernel=3, padding=1), (2, 8, 8, 8, 32), (32, 32, *k3), rowvec=1, res=(2, 8, 8, 8, 32))
    case("conv k3 s2 p1 sub-pixel dgrad", dt, conv(kernel=3, stride=2, padding=1), (2, 8, 8, 8, 32), (64, 32, *k3))
    case("conv k3 s2 pads (0, 1)", dt, conv(kernel=3, stride=2, padding=0, pad_hi=1), (2, 8, 8, 8, 32), (64, 32, *k3))
    case("conv k3 s2 p1 odd extents", dt, conv(kernel=3, stride=2, padding=1), (2, 6, 7, 9, 32), (64, 32, *k3))
    case("conv 2-D k3 s2", dt, conv(kernel=3, stride=2, padding=1), (2, 8, 10, 32), (32, 32, 3, 3))
    case("conv k4 s2 p1 1->32 relu", dt, conv(kernel=4, stride=2, padding=1, post_act="relu"), (2, 8, 8, 8, 1), (32, 1, 4, 4, 4))
    case("conv k1", dt, conv(kernel=1), (2, 4, 4, 4, 32), (64, 32, 1, 1, 1))
    case("linear res", dt, lambda x, w, b, res: A.linear(x, w, b, res), (2, 24, 32), (96, 32), res=(2, 24, 96))
    case("conv_transpose k3 s2 p1 op1", dt, lambda x, w, b: A.conv_transpose(x, w, b, kernel=3, stride=2, padding=1, output_padding=1),
         (2, 4, 4, 4, 32), (32, 32, *k3), transposed=True)
    case("conv_transpose 2-D k4 s2 p1", dt, lambda x, w, b: A.conv_transpose(x, w, b, kernel=4, stride=2, padding=1), (2, 4, 6, 32), (32, 32, 4, 4),
         transposed=True)
    case("conv_dilated k3 s2 d2 p2", dt, lambda x, w, b: A.conv_dilated(x, w, b, kernel=3, stride=2, padding=2, dilation=2), (2, 8, 8, 8, 32), (32, 32, *k3))
    case("conv_dilated 2-D k3 s2 d2 p2", dt, lambda x, w, b: A.conv_dilated(x, w, b, kernel=3, stride=2, padding=2, dilation=2), (2, 8, 8, 32), (32, 32, 3, 3))
    case("conv_dilated 2-D d1 k4 s2 p1 3->32", dt, lambda x, w, b: A.conv_dilated(x, w, b, kernel=4, stride=2, padding=1), (2, 8, 8, 3), (32, 3, 4, 4))
    case("conv_dilated 2-D d1 k4 s1 p1 3->32", dt, lambda x, w, b: A.conv_dilated(x, w, b, kernel=4, stride=1, padding=1), (2, 8, 8, 3), (32, 3, 4, 4))
    case("conv_transpose_dilated k3 s2 d2 p2 op1 relu", dt,
         lambda x, w, b: A.conv_transpose_dilated(x, w, b, kernel=3, stride=2, padding=2, output_padding=1, dilation=2, post_act="relu"),
         (2, 4, 4, 4, 32), (32, 32, *k3), transposed=True)
    case("upsample_conv 3-D", dt, A.upsample_conv, (2, 4, 4, 4, 32), (32, 32, *k3))
    case("upsample_conv 2-D", dt, A.upsample_conv, (2, 4, 6, 32), (32, 32, 3, 3))

    # (not a convolution: autograd.silu's backward is the activation backward the convolutions use, from the pre-activation)
    gen = torch.Generator().manual_seed(7)
    xs = randn(gen, (2, 24, 32), dt)
    del CALLS[:]
    ys = A.silu(xs)
    ys.backward(torch.randn(ys.shape, generator=gen).to(DEV, dt))
    RESULTS[f"silu {str(dt).split('.')[-1]}"] = dict(sha=dict(y=sha(ys), dx=sha(xs.grad)), calls=list(CALLS))

from torch.utils.checkpoint import checkpoint

case("conv k3 s1 p1 relu under checkpoint", torch.float32, conv(kernel=3, padding=1, post_act="relu"), (2, 8, 8, 8, 32), (32, 32, 3, 3, 3),
     wrap=lambda run: checkpoint(run, use_reentrant=False))


def in_autocast(run):
    with gm.autocast(torch.bfloat16):
        return run()


case("conv k3 s1 p1 fp32 master weight in autocast", torch.bfloat16, conv(kernel=3, padding=1), (2, 8, 8, 8, 32), (32, 32, 3, 3, 3),
     wdtype=torch.float32, wrap=in_autocast)


def reducer_case():
    """One weight and one bias under an armed GradientReducer (one rank, the collective backend): the first step learns the used set, the later
    ones add the weight gradient into the bucket view (autograd._weight_grad)."""
    import torch.distributed as dist
    from generativemodels_amd.parallel import GradientReducer

    for k, v in dict(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1").items():
        os.environ.setdefault(k, v)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    gen = torch.Generator().manual_seed(21)
    w = torch.nn.Parameter(randn(gen, (32, 32, 3, 3, 3), torch.float32, 0.05, grad=False))
    b = torch.nn.Parameter(randn(gen, (32,), torch.float32, 0.1, grad=False))
    x = randn(gen, (2, 6, 6, 8, 32), torch.float32, grad=False)
    red = GradientReducer([w, b], bucket_mb=0.001, force=True)
    out = dict(sha={}, calls=[])
    for step in range(3):
        red.zero_grad()
        del CALLS[:]
        h = A.conv(x, w, b, kernel=3, padding=1)
        (A.conv(h, w, b, kernel=3, padding=1).float() ** 2).mean().backward()
        red.finish()
        torch.cuda.synchronize()
        out["sha"].update({f"dweight step {step}": sha(w.grad), f"dbias step {step}": sha(b.grad)})
        out["calls"] += [f"step {step}"] + list(CALLS)
    out["sha"]["in bucket"] = str(w.grad.data_ptr() == red._view[id(w)].data_ptr())
    red.close()
    dist.destroy_process_group()
    return out


try:
    RESULTS["two-parameter model under a GradientReducer"] = reducer_case()
except Exception as e:
    RESULTS["two-parameter model under a GradientReducer"] = dict(error=f"{type(e).__name__}: {e}", calls=list(CALLS))

errors = {k: v["error"] for k, v in RESULTS.items() if "error" in v}
with open(args.out, "w") as f:
    json.dump(RESULTS, f, indent=1, sort_keys=True)
print(f"{len(RESULTS)} cases, {sum(len(v['calls']) for v in RESULTS.values())} native calls, {len(errors)} raised -> {args.out}")
for k, v in errors.items():
    print(f"  RAISED {k}: {v}")
sys.exit(1 if errors else 0)
