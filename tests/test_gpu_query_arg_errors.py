"""What the 18 query entry points answer to faulty arguments, pinned case by case: tests/golden/query_arg_errors.json
holds the return code and the rtow_last_error() text that scripts/record_query_arg_errors.py recorded for every case of
query_arg_cases.py — single faults, and pairs of faults that show which check comes first — on a context without a scene
(phase 0) and with handmade_scene() resident (phase 1).  Every case is refused before anything is launched.
"""
import json

import pytest

import query_arg_cases as qa
import rtow
from conftest import GOLDEN
from support_scenes import handmade_scene

pytestmark = pytest.mark.gpu

TABLE = json.loads((GOLDEN / "query_arg_errors.json").read_text())


def test_table_holds_every_case():
    assert [(r["phase"], r["fn"], r["args"]) for r in TABLE] == [(p, fn, o) for p, fn, o in qa.cases()]
    assert {r["fn"] for r in TABLE} == set(qa.ENTRIES) and all(r["rc"] != rtow.RTOW_OK for r in TABLE)


@pytest.mark.parametrize("phase", [0, 1])
def test_argument_errors_are_the_recorded_ones(phase):
    L = rtow.lib()
    bufs = qa.Buffers()
    scene = handmade_scene()
    ctx = rtow.Context(0)
    try:
        if phase:
            ctx.upload(scene.c)
        for r in TABLE:
            if r["phase"] != phase:
                continue
            rc, err = qa.call(L, ctx._h, bufs, r["fn"], r["args"])
            assert rc != rtow.RTOW_OK, (r["fn"], r["args"])
            assert (rc, err) == (r["rc"], r["err"]), (r["fn"], r["args"])
    finally:
        ctx.close()
