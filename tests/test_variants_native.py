"""The native VCF reader (cropsr_amd/csrc/crp_variants.cpp) under ASan + UBSan: a stand-alone driver with its own main,
compiled from source with g++ the way tests/test_sanitizers.py builds its drivers (CPU, no preload)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variants_reader_fuzz_under_sanitizers(tmp_path):
    """600 seeded VCF files -- well-formed ones, the same with mutated bytes, byte soups -- through crp_variants_create /
    _add_bytes / _finish / _track whole, in random chunks and byte by byte, with random entry lists: the same statistics,
    error and track however the bytes are cut, tracks that keep the invariant, the capacity protocol, calls out of order."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "variants_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "variants_driver.cpp"), os.path.join(ROOT, "cropsr_amd", "csrc", "crp_variants.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
