"""Host sanitizers over the SuperGlue family's host code: all six .hip files of the library
compile with -fsanitize=address,undefined on the host side only (-Xarch_host; the gfx950 code is
built as usual and never launched), and the stand-alone tests/sanitize/superglue_host_driver.cpp
(its own main) runs the packer, every size query and the host-side argument checks.  The
program is run directly: nothing is loaded into Python.  CPU only."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRCS = ("matcher", "matcher_pack", "runtime", "gemm", "pnp", "frame_ops", "superpoint",
        "superglue")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_superglue_host_code_under_asan_ubsan(tmp_path):
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined"]
    inc = ["-I", os.path.join(REPO, "onepose_amd", "csrc"), "-I", os.path.join(REPO, "include")]
    procs = []
    for f in SRCS:
        cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-fPIC", "-std=c++17",
               "-fno-omit-frame-pointer", *san, *inc, "-c",
               os.path.join(REPO, "onepose_amd", "csrc", f + ".hip"), "-o", str(tmp_path / (f + ".o"))]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-4000:]
    lib = str(tmp_path / "libonepose_sg_asan.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", *san, "-o", lib,
                        *[str(tmp_path / (f + ".o")) for f in SRCS]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    exe = str(tmp_path / "superglue_host_driver")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, "-I",
                        os.path.join(REPO, "include"),
                        os.path.join(HERE, "sanitize", "superglue_host_driver.cpp"),
                        "-o", exe, f"-L{tmp_path}", "-lonepose_sg_asan", f"-Wl,-rpath,{tmp_path}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-4000:]
    assert "runtime error" not in report and "AddressSanitizer" not in report, report[-4000:]
    assert "superglue size queries ok" in report
