"""Kernel routing of the training step, pinned call by call.

A route of ops.ConvGeom that silently stops applying falls back to the rows pass: the numbers stay right
and only the full-size benchmark would notice.  So this test records every lib.call of two training steps
(the second replays the batched weight packs) and compares the record with tests/golden/dispatch_steps64.json,
which was written by the commit before the dispatch refactor:

    python tests/test_gpu_dispatch.py OUT.json            the fixture
    python tests/test_gpu_dispatch.py --dump OUT.json     every trace's full records, for a field-level diff

Per call: the entry point; int / float arguments as they are; pointers as null / non-null; by-reference
output ints as "out"; of every ConvDesc all integer fields and whether rng_a, rng_b and b_h3 are null; of
dcs_pack_plan the input fields of its jobs.  lib.query calls launch nothing and are not recorded, nor is
dcs_range_arena_register: a stream's arena is registered once per process, so whether that falls inside a
trace depends on what ran before it.  The fixture keeps, per trace, the sequence of entry points and a
SHA-256 of the canonical full records (the full records of the sixteen traces pass 2 MB, their 800 distinct
ones 500 KB).

Traces: the soft-tissue (cin 3) and the lung (cin 2) model at 64 x 64 -- the smallest size at which the
residual convs reach the window kernel (W = 16) and the phase kernels tile -- in the operand modes f16x3,
f16, f32 and bf16x6, and in f16x3 with the selectors _WIN, _STEM, _WIN + _FUSE_FOLD and _SUBWIN off.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import GOLDEN
from oracle import prng

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(GOLDEN, "dispatch_steps64.json")

MODELS = {"soft": 3, "lung": 2}
# name -> (operand mode, selectors held off)
VARIANTS = {
    "f16x3": ("f16x3", ()),
    "f16": ("f16", ()),
    "f32": ("f32", ()),
    "bf16x6": ("bf16x6", ()),
    "f16x3-nowin": ("f16x3", ("_WIN",)),
    "f16x3-nostem": ("f16x3", ("_STEM",)),
    "f16x3-nowin-nofold": ("f16x3", ("_WIN", "_FUSE_FOLD")),
    "f16x3-nosubwin": ("f16x3", ("_SUBWIN",)),
}
# every route of the step has to show up in the fixture at least once
ROUTES = ("dcs_stem_fwd", "dcs_stem_wgrad", "dcs_head_fwd_proj", "dcs_head_wgrad_proj", "dcs_head_dgrad_in",
          "dcs_conv3_win_in_stats", "dcs_conv_dgrad_reflect_win", "dcs_conv_dgrad_reflect_win_inbwd",
          "dcs_subpix_win", "dcs_subpix_win_dgrad", "dcs_stride2_win", "dcs_phase_win_dgrad_inbwd",
          "dcs_conv_rows", "dcs_conv_rows_in_stats", "dcs_conv_dgrad_reflect", "dcs_reflect_fold",
          "dcs_conv_rows_narrow", "dcs_conv_wgrad", "dcs_conv_wgrad_narrow", "dcs_conv_dgrad_c1",
          "dcs_conv_dgrad_to1", "dcs_pack_batch")

_DESC_PTRS = ("rng_a", "rng_b", "b_h3")
_JOB_OUT = ("b0", "b1", "p0", "p1")  # written by dcs_pack_plan


def _null(v):
    return "null" if not v else "ptr"


def _struct(obj, ptr_fields, skip=()):
    out = []
    for f, _ in obj._fields_:
        if f not in skip:
            v = getattr(obj, f)
            out.append([f, _null(v) if (f in ptr_fields or v is None) else v])
    return out


def _arg(lib, a, argtype):
    if a is None:
        return "null"
    obj = getattr(a, "_obj", None)  # ctypes.byref(...)
    if isinstance(obj, lib.ConvDesc):
        return {"desc": _struct(obj, _DESC_PTRS)}
    if obj is not None:
        return "out"
    if argtype is ctypes.c_void_p or isinstance(a, (ctypes.c_void_p, ctypes.Array)):
        return _null(a.value if isinstance(a, ctypes.c_void_p) else a)
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    raise TypeError(f"unrecorded argument {a!r}")


def _record(lib, name, args):
    types = lib.SIGNATURES[name][1]
    assert len(types) == len(args), (name, len(types), len(args))
    rec = [name] + [_arg(lib, a, t) for a, t in zip(args, types)]
    if name == "dcs_pack_plan":
        jobs = (lib.PackJob * args[1]).from_address(args[0])
        ptrs = [f for f, t in lib.PackJob._fields_ if t is ctypes.c_void_p]
        rec.append({"jobs": [_struct(j, ptrs, _JOB_OUT) for j in jobs]})
    return rec


def trace(cin, variant):
    """The recorded lib.call sequence of two train steps of the ``cin`` model under ``variant``."""
    from modules.hip import lib, ops
    from test_gpu_concurrent import _batch
    from test_gpu_train import _system
    mode, off = VARIANTS[variant]
    z = np.load(os.path.join(GOLDEN, "steps_64.npz"))
    n, hw, nb, _, _, seed = [int(v) for v in z["meta"]]
    calls = []
    real_call = lib.call

    def recording_call(name, *args):
        if name != "dcs_range_arena_register":
            calls.append(_record(lib, name, args))
        return real_call(name, *args)

    prev_mma = ops.get_mma()
    prev_sel = {k: getattr(ops, k) for k in off}
    torch.cuda.synchronize()
    ops._WS.clear()  # workspace sizes are arguments: start every trace from the same (empty) scratch
    try:
        ops.set_mma(mode)
        for k in off:
            setattr(ops, k, False)
        s = _system(cin, nb, prng.step_model_seeds(seed))
        batches = [_batch(seed, i, n, hw, cin) for i in range(2)]
        lib.call = recording_call
        for b in batches:
            s.train_step(*b)
        torch.cuda.synchronize()
    finally:
        lib.call = real_call
        for k, v in prev_sel.items():
            setattr(ops, k, v)
        ops.set_mma(prev_mma)
    return calls


def summarise(calls):
    """What the fixture keeps of a trace: the entry points in order (as indices into their sorted set) and
    a hash of the canonical full records."""
    names = sorted({c[0] for c in calls})
    idx = {nm: i for i, nm in enumerate(names)}
    canon = json.dumps(calls, sort_keys=True, separators=(",", ":"))
    return {"names": names, "seq": [idx[c[0]] for c in calls], "sha256": hashlib.sha256(canon.encode()).hexdigest()}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_route(golden):
    seen = {nm for t in golden.values() for nm in t["names"]}
    assert not [r for r in ROUTES if r not in seen]
    assert sorted(golden) == sorted(f"{m}/{v}" for m in MODELS for v in VARIANTS)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("model", list(MODELS))
def test_dispatch_matches_parent(golden, model, variant):
    want = golden[f"{model}/{variant}"]
    got = summarise(trace(MODELS[model], variant))
    got_names = [got["names"][i] for i in got["seq"]]
    want_names = [want["names"][i] for i in want["seq"]]
    first = next((i for i, (a, b) in enumerate(zip(got_names, want_names)) if a != b), None)
    assert first is None, (first, got_names[max(first - 3, 0):first + 3], want_names[max(first - 3, 0):first + 3])
    assert len(got_names) == len(want_names)
    # same entry points in the same order: the arguments differ if this fails (--dump gives the fields)
    assert got["sha256"] == want["sha256"]


if __name__ == "__main__":
    dump = "--dump" in sys.argv
    path = [a for a in sys.argv[1:] if a != "--dump"][0]
    out = {}
    for m, cin in MODELS.items():
        for v in VARIANTS:
            calls = trace(cin, v)
            out[f"{m}/{v}"] = calls if dump else summarise(calls)
            print(m, v, len(calls), "calls", flush=True)
    if not dump:
        seen = {nm for t in out.values() for nm in t["names"]}
        missing = [r for r in ROUTES if r not in seen]
        assert not missing, f"routes not reached: {missing}"
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
