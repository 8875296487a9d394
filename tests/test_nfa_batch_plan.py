"""The host arithmetic of a batch of automaton searches (femto_amd/csrc/nfa_batch.hpp: validation, flattening, the kernel's LDS
plan, the order, the arena and the clock of a pass, grouping and sorting the raw ranges) on the CPU: tests/nfa_batch_check.cpp, a
stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer and run once."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_nfa_batch_host_arithmetic(tmp_path):
    exe = str(tmp_path / "nfa_batch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "nfa_batch_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "nfa_batch ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
