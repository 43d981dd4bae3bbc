"""build.dependencies(): the staleness check follows the source's own #include lines, so a header nobody listed by hand cannot
leave a stale library loaded.  No compile, no GPU."""

import os
import re
import shutil
import time

import pytest

from codd_query_engine_amd import build as b

INCLUDE = os.path.join(b._ROOT, "include")
PARTS = ["ingest_kernels.h", "scan_kernels.h", "shadow8_kernels.h", "list_scan_kernels.h", "dispatch.h"]


def walk_includes(start):
    """An independent walk: every file reached from `start` through #include "..." lines, looked up beside the including file,
    under csrc/ and under include/."""
    reached, todo = set(), [start]
    while todo:
        path = todo.pop()
        if path in reached:
            continue
        reached.add(path)
        for line in open(path, encoding="utf-8"):
            m = re.match(r'\s*#\s*include\s*"([^"]+)"', line)
            if not m:
                continue
            hits = [p for p in (os.path.join(d, m.group(1)) for d in (os.path.dirname(path), b.CSRC, INCLUDE)) if os.path.isfile(p)]
            assert hits, f'{path} includes "{m.group(1)}", which is nowhere'
            todo.append(os.path.realpath(hits[0]))
    return reached


def test_dependencies_hold_everything_the_source_includes():
    deps = b.dependencies()
    assert all(os.path.isabs(d) and os.path.isfile(d) for d in deps), deps
    assert len(deps) == len(set(deps))
    got = {os.path.realpath(d) for d in deps}
    want = walk_includes(os.path.realpath(os.path.join(b.CSRC, "codd_knn.hip")))
    assert want <= got, sorted(want - got)
    assert os.path.realpath(os.path.join(INCLUDE, "codd_knn.h")) in got


def test_no_header_under_csrc_is_an_orphan():
    got = {os.path.realpath(d) for d in b.dependencies()}
    on_disk = {os.path.realpath(os.path.join(b.CSRC, f)) for f in os.listdir(b.CSRC) if f.endswith((".h", ".inc"))}
    assert {os.path.realpath(os.path.join(b.CSRC, p)) for p in PARTS} <= on_disk
    assert on_disk <= got, sorted(on_disk - got)


@pytest.fixture()
def tree(tmp_path, monkeypatch):
    """A copy of csrc/ (text only) and include/ with a library that is newer than every file the real check looks at."""
    csrc, inc = tmp_path / "csrc", tmp_path / "include"
    shutil.copytree(b.CSRC, csrc, ignore=lambda d, names: [n for n in names if not n.endswith((".hip", ".h", ".inc"))])
    shutil.copytree(INCLUDE, inc)
    lib = csrc / "libcodd_knn.so"
    lib.write_bytes(b"")
    built = time.time() + 1000.0
    os.utime(lib, (built, built))
    monkeypatch.setattr(b, "CSRC", str(csrc))
    monkeypatch.setattr(b, "INCLUDE", str(inc))
    monkeypatch.setattr(b, "LIB_PATH", str(lib))
    return csrc, inc, built


@pytest.mark.parametrize("name", PARTS + ["filter_gemm_body.inc", "codd_knn.h", "codd_knn.hip"])
def test_touching_a_dependency_makes_the_library_stale(tree, name):
    csrc, inc, built = tree
    assert not b._stale()
    path = (inc if name == "codd_knn.h" else csrc) / name
    os.utime(path, (built + 1000.0, built + 1000.0))
    assert b._stale()
