"""The host planning layer (keras_unsupervised_amd/csrc/kurbm_plan.h): split-K plans, workspace layouts and the plane formats of
the x3 step are plain C++ that needs no device, so they are pinned on the CPU.

tests/golden/host_plans.json.xz records what the single-file host layer this header was split out of computed (commit 143d184,
"Discriminative and hybrid training of label RBMs on a new HIP kernel"): tests/dump_host_plans.cpp was compiled in one translation
unit with that commit's kurbm_api.hip, behind shims that gave its static planners and carvers the names of kurbm_plan.h and copied
its inline expressions (the format flags of cd_step_any, the plane choice of kurbm_x3_dump_plane, the layout of
kurbm_free_energy_x3), with a context filled by hand: CU count, knob defaults, no override.  The same program against the header
must print the same integers, key for key; a change of a size, a plan or a format is a change of the C ABI's contract and needs a
new fixture with its reason."""
import ctypes as C
import json
import lzma
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "keras_unsupervised_amd", "csrc")
V_BINARY = 0x10


@pytest.fixture(scope="module")
def golden(golden_dir):
    with lzma.open(os.path.join(golden_dir, "host_plans.json.xz"), "rt") as f:
        return json.load(f)


def test_plans_layouts_and_formats_match_the_fixture(tmp_path, golden):
    """g++ -std=c++17, no HIP: the header is host-only.  Every record and every field, exactly (they are integers)."""
    exe = tmp_path / "dump_host_plans"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "dump_host_plans.cpp"),
                    "-o", str(exe)], check=True)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert len(golden) > 9000
    assert sorted(got) == sorted(golden)
    wrong = [k for k in golden if got[k] != golden[k]]
    assert not wrong, "%d records differ, first: %s: %r, fixture %r" % (len(wrong), wrong[0], got[wrong[0]], golden[wrong[0]])


def test_fixture_holds_the_grid_edges(golden):
    """The thinned cross product still names every row count, every shape, both CU counts and every knob setting."""
    keys = list(golden)
    for rows in (1, 4, 31, 32, 33, 64, 100, 127, 128, 129, 512, 513, 4096):
        assert any("|r=%d," % rows in k for k in keys), rows
    for nv, nh in ((1, 1), (16, 8), (128, 128), (129, 64), (130, 260), (784, 1024), (794, 1024), (1024, 784), (4096, 4096)):
        for ncu in (256, 32):
            assert any(k.startswith("ncu=%d|default|" % ncu) and ",v=%d,h=%d|" % (nv, nh) in k for k in keys), (ncu, nv, nh)
    for knob in ("KURBM_SPLIT=2", "KURBM_CFG_OUTER=1", "KURBM_BF16_SPLIT=3", "KURBM_X3_SPLIT_STATS=0", "KURBM_X3_STATS_TALL=0",
                 "KURBM_X3_BYTES=0", "KURBM_LDPAD=8"):
        assert sum(1 for k in keys if "|%s|" % knob in k and "|plan_outer" in k and "one" not in k) == 3, knob
        assert sum(1 for k in keys if "|%s|formats|" % knob in k) == 3 * 3 * 2, knob
    assert sum(1 for k in keys if "|stats.pl|" in k and "lo=640,hi=784" in k) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,n_vis,n_hid", [(4, 16, 8), (100, 130, 260), (128, 784, 1024)])
def test_live_context_reports_the_fixture_sizes(gpu_device, golden, rows, n_vis, n_hid):
    """Ties the hand-filled context of the CPU test to what kurbm_ctx_create builds: on a fresh context with no knob set, the public
    *_bytes functions return the fixture's sizes for 256 CUs and default knobs.  No kernel is launched beyond the context's own."""
    import torch
    from keras_unsupervised_amd import _lib
    ncu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    knobs_set = sorted(k for k in os.environ if k.startswith("KURBM_") and k not in ("KURBM_LIB", "KURBM_PEER_TIMEOUT_MS"))
    print("device reports %d CUs; KURBM_* environment: %s" % (ncu, knobs_set or "none"))
    if ncu != 256 or knobs_set:
        print("NOT an MI355X with default knobs: the fixture has no row for this context, nothing compared")
        return
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.kurbm_ctx_create(gpu_device.index, C.byref(h)))
    try:
        def rec(what, tag=""):
            return golden["ncu=256|default|r=%d,v=%d,h=%d|%s%s" % (rows, n_vis, n_hid, what, "|" + tag if tag else "")]
        assert lib.kurbm_workspace_bytes(h, rows, n_vis, n_hid, 1) == rec("carve_f32", "ldv=0")["bytes"]
        assert lib.kurbm_class_workspace_bytes(h, rows, n_vis, n_hid) == rec("carve_class")["bytes"]
        assert lib.kurbm_ais_workspace_bytes(h, rows, n_vis, n_hid) == rec("carve_ais")["bytes"]
        for c in (2, 10, 64):
            if c < n_vis:
                assert lib.kurbm_disc_workspace_bytes(h, rows, n_vis, n_hid, c) == rec("carve_disc", "C=%d,ldv=0" % c)["bytes"]
        assert lib.kurbm_bf16_mirror_bytes(h, n_vis, n_hid) == rec("carve_mirror", "pieces=1")["bytes"]
        assert lib.kurbm_x3_mirror_bytes(h, n_vis, n_hid) == rec("carve_mirror", "pieces=3")["bytes"]
        assert lib.kurbm_bf16_workspace_bytes(h, rows, n_vis, n_hid, 1) == rec("carve_bf16", "pieces=1,vp=1")["bytes"]
        for vp in (1, 1 | V_BINARY, 3):
            assert lib.kurbm_x3_workspace_bytes(h, rows, n_vis, n_hid, 1, vp) == rec("carve_bf16", "pieces=3,vp=%d" % (vp & 3))["bytes"]
            assert lib.kurbm_x3_planes_bytes(h, rows, n_vis, vp) == rec("carve_vplanes", "vp=%d" % (vp & 3))["bytes"]
            for mode in (0, 1):
                assert (lib.kurbm_gibbs_workspace_bytes(h, rows, n_vis, n_hid, vp, mode)
                        == rec("carve_gibbs", "vp=%d,mode=%d,clamp=0" % (vp, mode))["bytes"])
    finally:
        lib.kurbm_ctx_destroy(h)
