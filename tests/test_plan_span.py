"""The span arithmetic of plan_stream_kernel (femto_amd/plan/plan_span.hpp) on the CPU: tests/plan_span_check.cpp, a stand-alone
program, built with AddressSanitizer and UndefinedBehaviorSanitizer and run once."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_plan_spans_tile_the_batch(tmp_path):
    exe = str(tmp_path / "plan_span_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "plan_span_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "plan_span ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
