"""The block-wise step from a Python-free host: tests/host/host_blocked_c99.c, plain C99 against include/allegro_amd.h
("Frames larger than the workspace").  It steps the reference's ghost-atom frame (tests/golden/model_c2_ghost.npz) whole, as one block and
in blocks of a few atoms through the plain ABI and compares the three; CPU: it compiles against the shipped header; GPU: it runs."""
import os
import subprocess

import pytest
import torch

from tests.hip_utils import ROOT, model_from_fixture
from tests.test_host_programs import HOST_DIR, PKG, _write_frame
from tests.test_pair_allegro import load_ghost_fixture


def _build(out):
    cmd = ["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(HOST_DIR, "host_blocked_c99.c"), "-o", out, "-L", PKG, "-lallegro_amd", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_blocked_host_compiles_against_the_shipped_header(tmp_path):
    from allegro_amd.build import build_library

    build_library(verbose=False)
    assert os.path.getsize(_build(str(tmp_path / "host_blocked_c99"))) > 0


@pytest.mark.gpu
def test_blocked_c99_host_agrees_with_its_own_unblocked_call(tmp_path):
    from allegro_amd.build import build_library
    from allegro_amd.export import write_host_model

    build_library(verbose=False)
    gx = load_ghost_fixture(torch.float32)
    m = model_from_fixture(gx["base"], torch.float32)
    model_path, frame_path = str(tmp_path / "c2.aamodel"), str(tmp_path / "c2_ghost.frame")
    write_host_model(m, model_path)
    _write_frame(frame_path, gx, sort_by_center=True)
    exe = _build(str(tmp_path / "host_blocked_c99"))
    r = subprocess.run([exe, model_path, frame_path, "5e-5"], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "host_blocked_c99: OK" in r.stdout, r.stdout + r.stderr
    assert "one block == whole frame, bit for bit" in r.stdout
    assert "aa_model_check = -1" in r.stdout and "wrong cut for block 0" in r.stdout  # the wrong cut was reported, not swallowed
