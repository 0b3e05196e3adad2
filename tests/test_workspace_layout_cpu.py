"""CPU: the workspace layouts and the shared refusals of libnof.so's host entry points (csrc/host_entry.h).

Every nof_*_workspace_bytes export and the thirteen values of nof_field_workspace_offsets are compared,
exactly, with tests/golden/workspace_layouts.json, which was recorded once from a build of the commit its
header names and is never rewritten from the tree under test: refused inputs (0), the smallest legal
shapes, shapes whose parts are no multiple of 256 bytes, and one shape past 2^32 bytes per export whose
guards allow one (all but nearest and mesh volume, whose block counts are capped). Then the pointer tables
that no other CPU test walks entry by entry, the two null-descriptor refusals, and the sanitized
stand-alone check of the header itself. No call here reaches a HIP call: each is refused before it."""
import ctypes
import json
import os
import subprocess

import pytest

from bundlesdf_amd import _lib
from bundlesdf_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "workspace_layouts.json")) as _f:
    GOLDEN = json.load(_f)
EINVAL = 1
DUMMY = 0x1000      # a non-null address that is never read: every call below is refused first


def test_the_golden_file_covers_every_size_export():
    exports = {n for n in _lib.declared_symbols() if n.endswith("_workspace_bytes")}
    assert exports == set(GOLDEN["bytes"]) and len(exports) == 13
    assert "dc5a9bb" in GOLDEN["header"]
    capped = {"nof_nearest_workspace_bytes", "nof_mesh_volume_workspace_bytes"}      # at most 1024 blocks' partials
    for fn, rows in GOLDEN["bytes"].items():
        assert len(rows) >= 4, fn
        assert fn in capped or max(want for _, want in rows) > 1 << 32, fn      # a product formed in 32 bits shows


@pytest.mark.parametrize("fn", sorted(GOLDEN["bytes"]))
def test_workspace_bytes_equal_the_recorded_values(fn):
    L = _lib.lib()
    for args, want in GOLDEN["bytes"][fn]:
        assert getattr(L, fn)(*args) == want, (fn, args)


def test_field_workspace_offsets_equal_the_recorded_values():
    L = _lib.lib()
    assert len(GOLDEN["field_offsets"]) == len(GOLDEN["bytes"]["nof_field_workspace_bytes"])
    for args, want in GOLDEN["field_offsets"]:
        buf = (ctypes.c_uint64 * 14)(*([0xdead] * 14))
        assert L.nof_field_workspace_offsets(*args, buf, 13) == 0, args
        assert list(buf[:13]) == want and len(want) == 13, args
        assert buf[13] == 0xdead                                   # nothing past the thirteen values
        assert want[12] == L.nof_field_workspace_bytes(*args) and want == sorted(want) and want[0] == 0
    buf = (ctypes.c_uint64 * 13)()
    for args in ((-1, 32, 1, buf, 13), (1, 0, 1, buf, 13), (1, 32, 1, None, 13), (1, 32, 1, buf, 12)):
        assert L.nof_field_workspace_offsets(*args) == EINVAL
        assert b"field_workspace_offsets: bad R=" in L.nof_last_error()


def _fill(desc, **kw):
    for k, v in kw.items():
        setattr(desc, k, v)
    return desc


def _lift(L, ptrs):
    d = _fill(_lib.FrameLiftDesc(), N=1, H=4, W=4, P=1, M=2, **ptrs)
    return L.nof_frame_lift_matches(ctypes.byref(d), None)


def _covis(L, ptrs):
    d = _fill(_lib.FrameCovisDesc(), N=2, H=4, W=4, Q=1, stride=1, **ptrs)
    return L.nof_frame_covisibility(ctypes.byref(d), None)


def _mc_count(L, p):
    return L.nof_marching_cubes_count(p.get("volume"), 4, 4, 4, 0.0, p.get("tables"), p.get("cells"), p.get("block_counts"),
                                      p.get("block_range"), None)


def _mc_emit(L, p):
    return L.nof_marching_cubes_emit(p.get("volume"), 4, 4, 4, 0.0, p.get("tables"), p.get("cells"), p.get("block_base"), 3, 1,
                                     p.get("vertices"), p.get("faces"), None)


def _vertex_color(L, p):
    return L.nof_vertex_color_accumulate(p.get("zbuf"), 4, 4, p.get("mask"), 0.1, p.get("colors"), p.get("cam_in_ob"),
                                         p.get("ob_in_cam"), p.get("K"), p.get("V"), 5, 0.01, p.get("color_sum"),
                                         p.get("count"), None, None, None)


# entry point -> (call, its pointer table in refusal order); every entry is needed at the shapes used
TABLES = {
    "frame_lift_matches": (_lift, ["points", "normals", "pair_frames", "pair_start", "uv_a", "uv_b", "pts_a", "pts_b",
                                   "normals_a", "normals_b", "valid"]),
    "frame_covisibility": (_covis, ["points", "normals", "pairs", "T", "counts"]),
    "marching_cubes_count": (_mc_count, ["volume", "tables", "cells", "block_counts", "block_range"]),
    "marching_cubes_emit": (_mc_emit, ["volume", "tables", "cells", "block_base", "vertices", "faces"]),
    "vertex_color_accumulate": (_vertex_color, ["zbuf", "mask", "colors", "cam_in_ob", "ob_in_cam", "K", "V", "color_sum",
                                                "count"]),
}


@pytest.mark.parametrize("fn,index", [(fn, i) for fn, (_, names) in TABLES.items() for i in range(len(names))])
def test_each_tabled_pointer_is_refused_by_name(fn, index):
    """Entries before `index` set, entry `index` null: the refusal names that entry, whatever follows it."""
    L = _lib.lib()
    call, names = TABLES[fn]
    for rest in (0, DUMMY):      # the entries after it null, then set
        ptrs = {n: DUMMY for n in names[:index]}
        ptrs.update({n: rest for n in names[index + 1:] if rest})
        assert call(L, ptrs) == EINVAL
        assert L.nof_last_error() == f"{fn}: {names[index]} is NULL".encode()


@pytest.mark.parametrize("fn,name", [("nof_field_step", "field_step"), ("nof_quad_mirror", "quad_mirror")])
def test_a_null_descriptor_is_refused(fn, name):
    L = _lib.lib()
    assert getattr(L, fn)(None, None) != 0
    assert L.nof_last_error() == f"{name}: desc is NULL".encode()


def test_host_entry_header_under_the_host_sanitizers(tmp_path):
    """tests/host_entry_check.cpp: the carver's parts stay inside a buffer of exactly the reported size."""
    exe = str(tmp_path / "host_entry_check")
    cmd = [B.HIPCC, "-x", "hip", "-std=c++17", f"--offload-arch={B.ARCH}", "-O1", "-g", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "host_entry_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_entry_check: ok" in r.stdout, r.stdout + r.stderr
