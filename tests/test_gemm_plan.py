"""GEMM tile selection (csrc/gemm_plan.cpp) on the CPU: the planner is plain host code, so which tile runs which GEMM is
checked without a GPU.  tests/golden/gemm_tile_choices.txt holds the problems the product and the kernel tests launch --
every encoder GEMM of the five model widths at batch 1 / 2 / 4 / 8 with and without other lanes, the decoder's image-side
GEMMs, the weights loader's, and every forced tile on its test shapes plus shapes it must refuse -- with the tile the
picker chose before it moved out of kernels/gemm.hip.  tests/gemm_plan_choices.cpp (built here with the host compiler)
reports every line for which gemm_plan.cpp answers differently."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dlimgedit_amd" / "csrc"
CHOICES = ROOT / "tests" / "golden" / "gemm_tile_choices.txt"


def _host_compiler():
    rocm_clang = Path("/opt/rocm/lib/llvm/bin/clang++")
    cxx = str(rocm_clang) if rocm_clang.exists() else (shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    assert cxx, "no host C++ compiler found"
    return cxx


def test_gemm_plan_chooses_the_recorded_tiles(tmp_path):
    exe = tmp_path / "gemm_plan_choices"
    # gemm_plan.cpp needs nothing of HIP but the headers kernels.hpp names
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{CSRC}",
           str(ROOT / "tests" / "gemm_plan_choices.cpp"), str(CSRC / "gemm_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    problems = [l for l in CHOICES.read_text().splitlines() if l and not l.startswith("#")]
    assert len(problems) >= 600
    r = subprocess.run([str(exe), str(CHOICES)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-1000:]
    assert r.stdout.strip().splitlines()[-1] == f"{len(problems)} problems, 0 differ", r.stdout[-4000:]
