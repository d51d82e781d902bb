"""LocalBA's host plan (csrc/lba_plan.h: index structures, Schur items and units, arena layout, staging, window descriptors, task
lists, the continuation region's bound) in a stand-alone program of its own (tests/cpp/lba_plan_check.cpp), built with
-fsanitize=address,undefined and run on the CPU.  The program allocates the staging buffer and the arena at exactly the planned
sizes, walks every LbaWin through its own pointers and asserts what the plan's comments promise, on the smallest windows at which
each branch of the plan exists, under both landmark layouts.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "active-orb-slam2_amd", "csrc")


def test_the_plan_header_is_plain_host_cpp(tmp_path):
    """lba_plan.h (and lba_window.h behind it) compiles under g++ with no HIP include path"""
    src = tmp_path / "only_the_plan.cpp"
    src.write_text('#include "lba_plan.h"\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])


def test_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """(-fno-var-tracking: the sanitizers' reports name functions and lines, which -g alone gives; tracking the variables' locations
    through the instrumented code costs 6 of 14 s of this compile and nothing reads them)"""
    exe = str(tmp_path / "lba_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-var-tracking", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "lba_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
