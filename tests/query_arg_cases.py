"""The argument-error cases of the 18 query entry points (the nine device / host pairs of include/rtow.h), as data.

A case is (phase, entry point, overrides): phase 0 runs on a context without a scene, phase 1 with handmade_scene()
resident.  `call` makes the call with every argument valid — n = 1, k = 1, live buffers, a 2 x 1 image of one sample —
except what the overrides name:
    an integer argument (precision, kernel, n, k, max_hits)   its value
    a buffer                                                  "null", or "off1": one byte into the live allocation
    params                                                    "null", or {field: value}
    cfg                                                       "null", or {field: value}
Every case but phase 0's all-valid call carries at least one fault that is refused before anything is launched, and every
buffer is 4 KiB (two records of any kind and more), so not even a check that wrongly passed could reach unowned memory.
scripts/record_query_arg_errors.py records what a build answers (tests/golden/query_arg_errors.json);
test_gpu_query_arg_errors.py replays the table.
"""
import ctypes as C

import rtow

BUF_BYTES = 4096

# entry point -> its arguments behind ctx, in ABI order: (name, kind[, alignment of a device buffer | maximum of k])
_PK = [("precision", "int"), ("kernel", "int")]
_TAIL_D, _TAIL_H = [("stream", "zero"), ("stats", "zero")], [("stats", "zero")]


def _pair(name, args, stats=True):
    """The device and the host form: the same arguments, the device form with alignments and a stream."""
    host = [(a[0], a[1]) if a[1] in ("req", "opt") else a for a in args]
    return {f"rtow_{name}_device": args + (_TAIL_D if stats else [("stream", "zero")]),
            f"rtow_{name}": host + (_TAIL_H if stats else [])}


ENTRIES = {
    **_pair("intersect", _PK + [("rays", "req", 16), ("n", "int"), ("hits", "req", 8)]),
    **_pair("occluded", _PK + [("rays", "req", 16), ("n", "int"), ("occluded", "req", 1)]),
    **_pair("closest_point", _PK + [("queries", "req", 16), ("n", "int"), ("hits", "req", 16)]),
    **_pair("first_hits", _PK + [("rays", "req", 16), ("n", "int"), ("max_hits", "k", rtow.MAX_HITS), ("hits", "req", 8),
                                 ("counts", "opt", 4)]),
    **_pair("nearest", _PK + [("queries", "req", 16), ("n", "int"), ("k", "k", rtow.MAX_NEAREST), ("hits", "req", 16),
                              ("counts", "opt", 4)]),
    **_pair("radiance", _PK + [("params", "radiance"), ("rays", "req", 16), ("n", "int"), ("ids", "opt", 8),
                               ("rgb", "req", 8)]),
    **_pair("path_step", _PK + [("params", "step"), ("rays", "req", 16), ("n", "int"), ("ids", "opt", 8),
                                ("next", "req", 16), ("atten", "req", 8), ("status", "req", 4), ("hits", "opt", 8)]),
    **_pair("camera_rays", [("cfg", "cfg"), ("rays", "req", 16), ("ids", "opt", 8)], stats=False),
    **_pair("guides", [("cfg", "cfg"), ("guides", "req", 16)]),
}
assert len(ENTRIES) == 18

REFTREE_REFUSED = ("rtow_first_hits", "rtow_closest_point", "rtow_nearest")  # at every precision


def cases():
    """[(phase, entry point, overrides)] in a fixed order."""
    out = []
    for phase in (0, 1):
        for fn, args in ENTRIES.items():
            device = fn.endswith("_device")
            camera = args[0][1] == "cfg"
            bufs = [a for a in args if a[1] in ("req", "opt")]
            required = [a[0] for a in bufs if a[1] == "req"]
            # what carries precision and kernel: the arguments themselves, or the config's fields
            field = (lambda k, v: {"cfg": {k: v}}) if camera else (lambda k, v: {k: v})
            c = []
            if phase == 0:
                c.append({})  # no scene
            if not camera:
                c += [{"n": -1}, {"n": 1 << 31}]
            c += [{b: "null"} for b in required]
            if device:
                c += [{b[0]: "off1"} for b in bufs if b[2] > 1]  # (a 1-byte alignment cannot be missed)
            c += [field("precision", rtow.F32), field("precision", 7), field("kernel", -2), field("kernel", 9)]
            if fn.removesuffix("_device") in REFTREE_REFUSED:
                c.append({"kernel": rtow.KERNEL_REFTREE, "precision": rtow.F64_STRICT})
            elif "camera_rays" not in fn:  # (rtow_camera_rays* resolve no strategy: REFTREE is no fault there)
                c.append(field("kernel", rtow.KERNEL_REFTREE))
            for a in args:
                if a[1] == "k":
                    c += [{a[0]: 0}, {a[0]: a[2] + 1}]
                if a[1] == "radiance":
                    c += [{"params": "null"}, {"params": {"samples_per_ray": 0}}, {"params": {"max_child_rays": -1}}]
                if a[1] == "step":
                    c += [{"params": "null"}, {"params": {"bounce": -1}}]
            if camera:
                c += [{"cfg": "null"}, {"cfg": {"image_width": 0}}]
            # two faults at once: which one is reported
            if "nearest" in fn:
                c.append({"k": 0, "n": -1})
            if "first_hits" in fn:
                c.append({"n": -1, "max_hits": 0})
            if device and len(bufs) > 1:
                later = [b[0] for b in bufs[1:] if b[1] == "req"] or [b[0] for b in bufs[1:]]
                c.append({bufs[0][0]: "off1", later[0]: "off1"})
            c.append({required[0]: "null", **field("precision", 7)})
            if "path_step" in fn:
                c.append({"params": {"bounce": -1}, "kernel": 9})
            if not camera:
                c.append({"n": 0, "precision": 7})
            out += [(phase, fn, o) for o in c]
    return out


class Buffers:
    """One live 4 KiB allocation per buffer argument name: device memory for the device forms, host memory otherwise."""

    def __init__(self):
        import numpy as np
        import torch

        names = sorted({a[0] for args in ENTRIES.values() for a in args if a[1] in ("req", "opt")})
        self.dev = {n: torch.zeros(BUF_BYTES, dtype=torch.uint8, device="cuda") for n in names}
        self.host = {n: np.zeros(BUF_BYTES, dtype=np.uint8) for n in names}

    def ptr(self, name, device):
        return self.dev[name].data_ptr() if device else self.host[name].ctypes.data


def call(L, ctx, bufs, fn, overrides):
    """(return code, rtow_last_error() text) of `fn` on the context handle `ctx` with the overrides applied."""
    device = fn.endswith("_device")
    argv, keep = [ctx], []
    for a in ENTRIES[fn]:
        name, kind = a[0], a[1]
        o = overrides.get(name)
        if kind == "int":
            argv.append(o if o is not None else {"precision": rtow.F64_FAST, "kernel": rtow.KERNEL_AUTO, "n": 1}[name])
        elif kind == "k":
            argv.append(o if o is not None else 1)
        elif kind in ("req", "opt"):
            p = bufs.ptr(name, device)
            argv.append(None if o == "null" else p + 1 if o == "off1" else p)
        elif kind == "zero":
            argv.append(None)
        else:
            if kind == "radiance":
                s = rtow.RadianceParams(1, 1, 4, 0, 0)
            elif kind == "step":
                s = rtow.StepParams(1, 0, 0)
            else:
                s = rtow.make_config(2, 1, 1, 1, 4)
            for k, v in (o.items() if isinstance(o, dict) else ()):
                setattr(s, k, v)
            keep.append(s)
            argv.append(None if o == "null" else C.byref(s))
    rc = getattr(L, fn)(*argv)
    return int(rc), (L.rtow_last_error() or b"").decode()
