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
                 "gm_stats_compact_slots", "gm_gn_channel_stats_slots", "gm_gn_workspace_bytes", "gm_last_error", "gm_abi_version",
                 # ... and the attention planners (tests/test_attention_routes.py): pure arithmetic on a descriptor
                 "gm_attention_backward_workspace_bytes", "gm_attention_backward_fused_workspace_bytes", "gm_attention_bwd_scores_workspace_bytes",
                 "gm_attention_workspace_bytes", "gm_attention_stats_slots", "gm_attention_max_head_dim", "gm_attention_max_wide_head_dim",
                 "gm_conv_wgrad_workspace_bytes",
                 # ... and the route of the row GEMMs (tests/test_rows_routes.py)
                 "gm_rows_gemm_route"}


class _Pointer(int):
    """A pointer argument recorded while named base tensors are registered: resolved by RecordingLibrary.named()."""


class RecordingLibrary:
    """Stands in for the native library: the host-side planners go through to it, every other entry point is NOT called -- the call is
    appended to `calls` as [name, argument, ...] and 0 returned.  A pointer argument is recorded as null / non-null, an integer or float as
    itself, a structure passed by reference as the list of its fields in declaration order (pointers again as booleans; a field that points at
    another structure as false or that structure's field list).
    Two options, both off by default:  `bases` = {name: tensor} -- a pointer into the storage of one of these tensors is recorded as
    [name, byte offset from the tensor's first element] (the first match in registration order; any other non-null pointer stays `true`) once
    named() has run;  `planner_returns` = {planner name: value} -- that host-side planner answers `value` instead of being asked."""

    def __init__(self, real, bases=None, planner_returns=None):
        self.real, self.calls, self.bases, self.planner_returns = real, [], bases, planner_returns or {}

    def _value(self, v, ctype):
        import ctypes as C
        if ctype is C.c_void_p:
            return bool(v) if self.bases is None else _Pointer(v or 0)
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer) and issubclass(ctype._type_, C.Structure):  # GmRowsDesc.gn: false, or the fields it points at
            return [self._value(getattr(v.contents, f), t) for f, t in ctype._type_._fields_] if v else False
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return [self._value(e, ctype._type_) for e in v]
        if isinstance(v, float):
            return float(C.c_float(v).value) if ctype is C.c_float else v
        return v

    def named(self, **more):
        """Resolves the recorded pointers against `bases` and `more` = tensors that were allocated before the first recorded call and are
        still alive (the gradients an entry point returns), and returns `calls`."""
        spans = []
        for name, t in {**self.bases, **more}.items():
            st = t.untyped_storage()
            spans.append((name, st.data_ptr(), st.data_ptr() + st.nbytes(), t.data_ptr()))

        def walk(v):
            if isinstance(v, _Pointer):
                return next(([name, v - first] for name, lo, hi, first in spans if lo <= v < hi), bool(v))
            return [walk(e) for e in v] if isinstance(v, list) else v
        self.calls[:] = walk(self.calls)
        return self.calls

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in self.planner_returns:
            return lambda *args: self.planner_returns[name]
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
    """`with conv_on_cpu() as rec:` -- ops.conv / ops.linear (and every other entry point of ops) accept CPU tensors and launch nothing;
    rec.calls lists what they would have launched.  Keyword arguments: the options of RecordingLibrary."""

    def __init__(self, **options):
        self.options = options

    def __enter__(self):
        from generativemodels_amd import _native as nat
        from generativemodels_amd import ops
        self.ops, self.keep = ops, (ops.require_device, ops._stream, ops.lib)
        rec = RecordingLibrary(nat.lib(), **self.options)
        ops.require_device, ops._stream, ops.lib = (lambda *ts: None), (lambda: 0), (lambda: rec)
        return rec

    def __exit__(self, *exc):
        self.ops.require_device, self.ops._stream, self.ops.lib = self.keep
        return False
