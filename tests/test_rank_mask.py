"""The mask arithmetic of the ballot rank (bspy_amd/csrc/bsk_rank.hpp: rank_from_ballots) on the CPU.

tests/rank_mask_check.cpp is a stand-alone program: it feeds the function the ballots of a
wave, for 8, 16 and 32 classes, and compares every active lane's rank with a brute-force count - all lanes in one
class, classes with 0, 1, 4, 5 and 9 members, a class that lives in the upper half only, and partial EXEC masks
(1 lane, 33 lanes, holes).  Built with AddressSanitizer and UBSan where the compiler has them; never loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_rank_from_ballots_matches_brute_force(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = os.path.join(ROOT, "tests", "rank_mask_check.cpp")
    exe = str(tmp_path / "rank_mask_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "san" in (r.stderr + r.stdout).lower():
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)     # a compiler without the sanitizer runtimes
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rank mask ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
