"""The host plan of a batch of boolean trees (femto_amd/bquery/bquery_plan.hpp: forest, range table, level schedule with every
call's arena offsets) on the CPU: tests/bquery_plan_check.cpp, a stand-alone program, built with AddressSanitizer and
UndefinedBehaviorSanitizer and run once."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_bquery_plan_places_every_call(tmp_path):
    exe = str(tmp_path / "bquery_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "bquery_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "bquery_plan ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
