"""The searches the result-set stack shares (femto_amd/common/ragged.hpp) on the CPU: tests/ragged_check.cpp, a stand-alone
program, built with AddressSanitizer and UndefinedBehaviorSanitizer and run once."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_ragged_searches_and_merge_path(tmp_path):
    exe = str(tmp_path / "ragged_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ragged_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ragged ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
