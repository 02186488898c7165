"""Shared helpers for the parity tests (test infrastructure)."""
import os

import torch

import restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_fixture(name):
    fx = torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)
    if fx.get("state_dict") is None and fx.get("shapes") is not None:
        fx["state_dict"] = R.synthetic_state_dict(fx["shapes"], seed=fx["synthetic_seed"])
    return fx


def cast_sd(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def maxabs(a, b):
    return (a.double() - b.double()).abs().max().item()


def assert_close(a, b, atol, rtol=0.0, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; max|err|={err.max().item():.3e} "
        f"(atol={atol:g}, rtol={rtol:g}), ref absmax={b.abs().max().item():.3e}")


# ---- route census of ops.conv on a machine without a GPU -----------------------------------------------------------------------------
# Host-side planners of the library: they run without a device, and ops.conv's decisions depend on their answers.
HOST_PLANNERS = {"gm_conv_cfg_tile", "gm_conv_lds_bytes", "gm_conv_stats_slots", "gm_conv_splitk_workspace_bytes", "gm_packed_conv_weight_elems",
                 "gm_stats_compact_slots", "gm_gn_channel_stats_slots", "gm_gn_workspace_bytes", "gm_last_error", "gm_abi_version"}


class RecordingLibrary:
    """Stands in for the native library: the host-side planners go through to it, every other entry point is NOT called -- the call is
    appended to `calls` as [name, argument, ...] and 0 returned.  A pointer argument is recorded as null / non-null, an integer or float as
    itself, a structure passed by reference as the list of its fields in declaration order (pointers again as booleans)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    @staticmethod
    def _value(v, ctype):
        import ctypes as C
        if ctype is C.c_void_p:
            return bool(v)
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return [RecordingLibrary._value(e, ctype._type_) for e in v]
        if isinstance(v, float):
            return float(C.c_float(v).value) if ctype is C.c_float else v
        return v

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in HOST_PLANNERS:
            return fn

        def record(*args):
            row = [name]
            for v, ctype in zip(args, fn.argtypes):
                obj = getattr(v, "_obj", None)
                if obj is not None:
                    row.append([self._value(getattr(obj, f), t) for f, t in obj._fields_])
                else:
                    row.append(self._value(v, ctype))
            self.calls.append(row)
            return 0
        return record


class conv_on_cpu:
    """`with conv_on_cpu() as rec:` -- ops.conv / ops.linear accept CPU tensors and launch nothing; rec.calls lists what they would have launched."""

    def __enter__(self):
        from generativemodels_amd import _native as nat
        from generativemodels_amd import ops
        self.ops, self.keep = ops, (ops.require_device, ops._stream, ops.lib)
        rec = RecordingLibrary(nat.lib())
        ops.require_device, ops._stream, ops.lib = (lambda *ts: None), (lambda: 0), (lambda: rec)
        return rec

    def __exit__(self, *exc):
        self.ops.require_device, self.ops._stream, self.ops.lib = self.keep
        return False
