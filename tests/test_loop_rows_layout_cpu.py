"""The LDS layout of k4_out_lrows on the host: rnaelem_amd/csrc/loop_rows_layout.h, the one function the
kernel takes its regions from and the launcher its byte count -- for blocks of 1, 8, 16 and 32 rows, L rows of 1 to 16 columns
and bands of 3, 50, 64 and 120 the regions do not overlap and are aligned, the total is what the launcher passes, what a
workgroup stages fits its region for every first row, and the bench's shape stays within the 32 768 bytes that five workgroups
per CU allow.  It runs in tests/loop_rows_layout_check.cpp, a stand-alone program built with -fsanitize=address,undefined that
checks by itself and must end clean."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rnaelem_amd", "csrc")
SRC = os.path.join(HERE, "loop_rows_layout_check.cpp")
EXE = os.path.join(HERE, "loop_rows_layout_check_asan")


def test_loop_rows_layout():
    deps = [SRC, os.path.join(CSRC, "loop_rows_layout.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", EXE, SRC])
    # (the leak check, which some sandboxes cannot start, is left out: the program's vectors are freed by their destructors)
    r = subprocess.run([EXE], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 5000, r.stdout[-500:]
