"""The layout of the test suite itself (no GPU): helpers live in support modules, and importing a module is free.

1. No file under tests/ or scripts/ imports a module whose name starts with `test_`: what two modules share is in a
   support module (support_scenes, support_oracle, support_tables, support_fixtures) or in the reference module it
   belongs to (exact_cases, point_cases, guides_ref, ...).
2. Importing any module of tests/ loads neither librtow.so nor liboracle.so and starts no process, so collection works
   on a checkout with nothing built (the session fixture `_built` of conftest.py builds the libraries afterwards).
"""
import ast
import subprocess
import sys

from conftest import REPO

TESTS = REPO / "tests"


def test_no_module_imports_a_test_module():
    bad = []
    for path in sorted(TESTS.rglob("*.py")) + sorted((REPO / "scripts").rglob("*.py")):
        for node in ast.walk(ast.parse(path.read_text(), str(path))):
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            else:
                continue
            bad += [f"{path.relative_to(REPO)}:{node.lineno}: {n}" for n in names if n.split(".")[0].startswith("test_")]
    assert not bad, "\n".join(bad)


CHILD = """
import importlib, subprocess, sys
sys.path.insert(0, sys.argv[1])
import conftest, orc, rtow

def refuse(what):
    def f(*a, **k):
        raise AssertionError(what + " at import")
    return f

rtow.lib, orc.lib = refuse("rtow.lib()"), refuse("orc.lib()")
subprocess.run, subprocess.Popen = refuse("subprocess.run"), refuse("subprocess.Popen")
for name in sys.argv[2:]:
    importlib.import_module(name)
loaded = [l.split()[-1] for l in open("/proc/self/maps") if l.rstrip().endswith(("librtow.so", "liboracle.so"))]
assert not loaded, loaded
"""


def test_importing_the_test_modules_loads_no_library_and_starts_no_process():
    """A fresh interpreter in which rtow.lib, orc.lib, subprocess.run and subprocess.Popen raise imports every module of
    tests/ by name (what collection does on a checkout with nothing built); neither library is mapped afterwards."""
    names = sorted(p.stem for p in TESTS.glob("*.py"))
    assert "test_gpu_refit" in names and "support_scenes" in names
    r = subprocess.run([sys.executable, "-c", CHILD, str(TESTS)] + names, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
