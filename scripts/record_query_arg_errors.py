#!/usr/bin/env python3
"""Records what the built library answers to the faulty calls of tests/query_arg_cases.py: return code and
rtow_last_error() text per case, first on a context without a scene, then with handmade_scene() resident.  Run it on the
commit whose behaviour is to be pinned (RTOW_LIB selects another build); tests/test_gpu_query_arg_errors.py replays the
table.  A case the library accepts (RTOW_OK) is a mistake in the case list: nothing is written.

   python scripts/record_query_arg_errors.py [--out tests/golden/query_arg_errors.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402,F401  (torch's runtime is loaded before librtow's, see rtow.lib)
import rtow  # noqa: E402
import query_arg_cases as qa  # noqa: E402
from support_scenes import handmade_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests/golden/query_arg_errors.json"))
    a = ap.parse_args()
    L = rtow.lib()
    bufs = qa.Buffers()
    scene = handmade_scene()
    rows = []
    for phase in (0, 1):
        ctx = rtow.Context(0)
        if phase:
            ctx.upload(scene.c)
        for p, fn, o in qa.cases():
            if p != phase:
                continue
            rc, err = qa.call(L, ctx._h, bufs, fn, o)
            if rc == rtow.RTOW_OK:
                sys.exit(f"phase {phase} {fn} {o}: accepted (RTOW_OK) — not a faulty call; nothing written")
            rows.append({"phase": phase, "fn": fn, "args": o, "rc": rc, "err": err})
        ctx.close()
    text = "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(f"{len(rows)} cases, {len(text)} bytes -> {a.out}")


if __name__ == "__main__":
    main()
