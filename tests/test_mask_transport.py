"""The mask transport plan (csrc/mask_transport.hpp) on the CPU: which road the masks of a request take from the
post-processing kernel to the caller -- mode, where the kernel writes, launches, copy commands and events in stream order,
the pieces the host waits for -- is decided by plain host code, so it is checked without a GPU.
tests/mask_transport_cases.cpp (built here with the host compiler) prints the plan of one request; every expectation below
is worked out by hand from the rules (layout: masks one after the other, each padded to 256 bytes, IoU floats behind them;
direct: one mask, or up to six while the other lanes are idle; staged otherwise), none is printed from the planner."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"

SMALL = 1000                    # padded to 1024
MIB = 1024 * 1024               # 1024 x 1024, its own padded size
BIG = 1800 * 1200               # 2 160 000, padded to 2 160 128
OFF1 = 1024                     # layout of (SMALL, MIB, BIG): offsets 0, OFF1, OFF2; end END3
OFF2 = 1024 + MIB               # 1 049 600
END3 = OFF2 + 2160128           # 3 209 728


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    exe = tmp_path_factory.mktemp("mask_transport") / "mask_transport_cases"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "mask_transport_cases.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        out = {}
        for line in r.stdout.splitlines():
            key, *values = line.split()
            out[key] = values
        for key in ("in_place", "piece_end", "reserve"):
            out[key] = [int(v) for v in out[key]]
        for key in ("launches", "iou_offset", "pieces_agree"):
            out[key] = int(out[key][0])
        out["mode"] = out["mode"][0]
        out["kernel_dst"] = [v if v == "caller" else int(v) for v in out["kernel_dst"]]
        return out

    def host(sizes, pinned=None, iou=0, idle=True, direct_allowed=True):
        pinned = pinned or [0] * len(sizes)
        return run("host", int(direct_allowed), int(idle), iou, *[f"{s}:{p}" for s, p in zip(sizes, pinned)])

    host.device = lambda sizes, kernel_writes_dst: run("device", int(kernel_writes_dst), *sizes)
    return host


def test_no_masks_nothing_is_planned(plan):
    p = plan([])
    assert p["mode"] == "none" and p["steps"] == [] and p["launches"] == 0 and p["piece_end"] == [] and p["reserve"] == [0, 0]


def test_one_mask_goes_direct_whatever_the_other_lanes_do(plan):
    p = plan([SMALL], iou=4, idle=False)
    assert p["mode"] == "direct" and p["launches"] == 1
    assert p["kernel_dst"] == [0] and p["in_place"] == [0]
    assert p["piece_end"] == [1024 + 16] and p["iou_offset"] == 1024 and p["reserve"] == [1040, 1040]
    assert p["steps"] == ["L0+1", "C:iou@0>pinned@1024#16", "E0"]


def test_one_mask_is_staged_when_direct_writes_are_switched_off(plan):
    p = plan([SMALL], iou=4, direct_allowed=False)
    assert p["mode"] == "staged" and p["launches"] == 1 and p["kernel_dst"] == [0] and p["in_place"] == [0]
    assert p["piece_end"] == [1040] and p["reserve"] == [1040, 1040]
    assert p["steps"] == ["L0+1", "C:iou@0>device@1024#16", "C:device@0>pinned@0#1040", "E0"]


def test_six_masks_go_direct_while_the_other_lanes_are_idle(plan):
    sizes = [SMALL, MIB, BIG, SMALL, MIB, BIG]
    ends = [OFF1, OFF2, END3, END3 + 1024, END3 + 1024 + MIB, 2 * END3]
    p = plan(sizes, iou=24, idle=True)
    assert p["mode"] == "direct" and p["launches"] == 6
    assert p["kernel_dst"] == [0] + ends[:5] and p["in_place"] == [0] * 6
    assert p["iou_offset"] == 2 * END3 and p["reserve"] == [2 * END3 + 96] * 2
    assert p["piece_end"] == ends[:5] + [2 * END3 + 96]
    # one launch and one event per mask; the IoU copy between the last launch and the last event
    assert p["steps"] == ["L0+1", "E0", "L1+1", "E1", "L2+1", "E2", "L3+1", "E3", "L4+1", "E4",
                          "L5+1", f"C:iou@0>pinned@{2 * END3}#96", "E5"]


@pytest.mark.parametrize("count, idle", [(6, False), (7, True), (2, False)])
def test_more_masks_or_busy_lanes_are_staged_in_one_launch(plan, count, idle):
    p = plan([SMALL] * count, idle=idle)
    assert p["mode"] == "staged" and p["launches"] == 1
    assert [s for s in p["steps"] if s.startswith("L")] == [f"L0+{count}"]
    assert p["kernel_dst"] == [1024 * i for i in range(count)]


def test_direct_with_some_destinations_pinned_keeps_the_layout_of_the_others(plan):
    p = plan([SMALL, MIB, BIG], pinned=[1, 0, 1])
    assert p["mode"] == "direct" and p["in_place"] == [1, 0, 1]
    assert p["kernel_dst"] == ["caller", OFF1, "caller"]           # mask 1 behind the padded size of mask 0, not at 0
    # no IoU predictions: no copy command, and the last piece ends where the masks do
    assert p["piece_end"] == [OFF1, OFF2, END3] and p["reserve"] == [END3, END3]
    assert p["steps"] == ["L0+1", "E0", "L1+1", "E1", "L2+1", "E2"]


def test_staged_with_every_destination_pinned_copies_each_mask_to_its_place(plan):
    p = plan([SMALL, MIB, BIG], pinned=[1, 1, 1], iou=12, idle=False)
    assert p["mode"] == "staged" and p["in_place"] == [1, 1, 1] and p["kernel_dst"] == [0, OFF1, OFF2]
    assert p["iou_offset"] == END3 and p["piece_end"] == [END3 + 48] and p["reserve"] == [END3 + 48] * 2
    assert p["steps"] == ["L0+3", f"C:iou@0>device@{END3}#48", f"C:device@0>caller0@0#{SMALL}", f"C:device@{OFF1}>caller1@0#{MIB}",
                          f"C:device@{OFF2}>caller2@0#{BIG}", f"C:device@{END3}>pinned@{END3}#48", "E0"]


def test_staged_with_one_destination_not_pinned_travels_in_pieces(plan):
    p = plan([SMALL, MIB, BIG], pinned=[0, 1, 0], iou=12, idle=False)
    assert p["mode"] == "staged" and p["in_place"] == [0, 0, 0] and p["kernel_dst"] == [0, OFF1, OFF2]
    # 3 209 776 bytes: three pieces (one per whole MiB, six at most) of 3 209 776 / 3 rounded up to 256 = 1 070 080
    assert p["piece_end"] == [1070080, 2140160, END3 + 48] and p["pieces_agree"] == 1
    assert p["steps"] == ["L0+3", f"C:iou@0>device@{END3}#48", "C:device@0>pinned@0#1070080", "E0",
                          "C:device@1070080>pinned@1070080#1070080", "E1", f"C:device@2140160>pinned@2140160#{END3 + 48 - 2140160}", "E2"]
    # the same whichever destination is the unpinned one
    assert plan([SMALL, MIB, BIG], pinned=[1, 1, 0], iou=12, idle=False)["steps"] == p["steps"]


def test_staged_without_iou_predictions(plan):
    p = plan([SMALL, SMALL], idle=False)
    assert p["piece_end"] == [2048] and p["iou_offset"] == 2048 and p["reserve"] == [2048, 2048]
    assert p["steps"] == ["L0+2", "C:device@0>pinned@0#2048", "E0"]


def test_piece_counts_agree_with_the_piece_cutter(plan):
    # tests/test_mask_pieces.py: five 1 MiB masks travel in five pieces, sixteen in six
    for count, pieces in ((5, 5), (16, 6)):
        p = plan([MIB] * count, idle=False)
        assert p["mode"] == "staged" and len(p["piece_end"]) == pieces and p["piece_end"][-1] == count * MIB
        assert p["pieces_agree"] == 1 and [s for s in p["steps"] if s.startswith("E")] == [f"E{i}" for i in range(pieces)]


def test_device_form(plan):
    sizes = [SMALL, MIB, BIG]
    same = plan.device(sizes, True)
    assert same["mode"] == "device_direct" and same["kernel_dst"] == ["caller"] * 3
    assert same["steps"] == ["L0+3"] and same["reserve"] == [0, 0] and same["piece_end"] == []
    other = plan.device(sizes, False)
    assert other["mode"] == "device_staged" and other["kernel_dst"] == [0, OFF1, OFF2]
    assert other["reserve"] == [END3, 0] and other["piece_end"] == [] and other["launches"] == 1
    assert other["steps"] == ["L0+3", f"C:device@0>peer0@0#{SMALL}", f"C:device@{OFF1}>peer1@0#{MIB}", f"C:device@{OFF2}>peer2@0#{BIG}"]
    assert plan.device([], False)["mode"] == "none"
