"""The ctx's lazy state slot (csrc/ctx_state.hpp; no GPU, no HIP): the header under the sanitizers as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc")


def test_sanitizer_program(tmp_path):
    """isdf::Lazy with a counting dummy state under AddressSanitizer (leaks included) and UBSan: an empty slot, make twice, reset and
    make again, a slot destroyed while holding, two slots destroyed in reverse order (nothing of it runs in the Python process)."""
    exe = str(tmp_path / "ctx_state_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "ctx_state_sanitize_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(" ok: ") == 4 and "FAILED" not in r.stdout, r.stdout
    print("\n" + r.stdout)
