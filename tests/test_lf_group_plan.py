"""Which pipeline jobs share one SIMT LF launch, and how many LF streams a process with Q hardware queues uses (jpegxl-rs_amd/csrc/lf_group_plan.h: PlanLfGroups,
LfStreamsForQueues): tests/lf_group_plan.cc checks both against their rules on hand-made key sequences — the cap, mixed keys, ineligible jobs, order, the empty list, the
clamp to kLfGroupMax; Q unset, 0, 1, 4, 8, 16, 32 and garbage.  Host only; the program is built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lf_group_plan_matches_its_specification(tmp_path):
    exe = str(tmp_path / "lf_group_plan")
    src = os.path.join(ROOT, "tests", "lf_group_plan.cc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "jpegxl-rs_amd", "csrc"), "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(out.stdout)
    sys.stderr.write(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
