"""csrc/bgzf_host.h compiled on its own: the block lister of every BGZF input path against a serial walk (tests/host/bgzf_list_check.cpp).
Host code only: no GPU, no engine library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_lister_agrees_with_a_serial_walk(tmp_path):
    """Empty buffer, one block, an EOF block between blocks, buffers cut 1 / 17 / 18 bytes into a header and inside a body (with and
    without may_cut), bytes that are no header, trailers claiming 65,537 and 65,536 bytes, an extra subfield, no BC subfield, an
    xlen past the buffer, and just over 32 MB walked by four threads (as it is: four lists taken; with false headers planted behind
    the quarter marks: one; parallel off: none).  The program checks all of it and says which line failed."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler on this machine (c++, g++, clang++ or $CXX)")
    exe = str(tmp_path / "bgzf_list_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "metamlst_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "bgzf_list_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
