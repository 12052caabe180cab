"""The dispatch plans (csrc/mg_plan.h) as a host-only program: tests/plan_check.cpp includes only the plan header,
defines the tuning slots itself, is built with the host compiler under AddressSanitizer and UBSan, and checks

  structure, over M x N x K x (bf16, fp32, split-bf16 fp32) x epilogue forms and a grid of convs, at default tuning
  and under slots NO_SLABS (5) = 1, GEMM_TILE (3) in {64, 128, 257}, CONV_TILE (2) in {64, 128, 256, 257}, SHORTK (9) =
  2 and DETERMINISTIC (11) = 1: every slab plan has splits >= 2 chunks of whole K steps that cover K with none empty,
  every tile is one the library builds for the dtype, split-bf16 and loader-transform GEMMs stay on 64^2; anchors: the
  shapes whose measurements are quoted next to the rules take the tile the comment says; the four shapes of
  test_modconv_fused_gpu.py::test_fused_default_large_tiles come out as one launch on 128^2 (twice) and 128 x 256
  (twice) -- the GPU test cannot see which tile ran.

No device and no library build is needed."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
