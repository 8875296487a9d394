"""The rank-policy rule, its two narrowings, the policy dispatcher and the decision of a direct count launch
(femto_amd/csrc/policy_dispatch.hpp, direct_launch.hpp) on the CPU: tests/policy_check.cpp, a stand-alone program, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run once."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_policy_rule_decision_and_dispatcher(tmp_path):
    exe = str(tmp_path / "policy_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "policy_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "policy ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
