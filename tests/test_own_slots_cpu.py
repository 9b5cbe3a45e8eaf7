"""A slot per sequence and the zeros it keeps (option own_slots) on the host: the plain functions of
rnaelem_amd/csrc/slot_sizing.h -- own_slots_fit around the edge of every budget, the slot mapping and the group sizes against the
arithmetic Engine::sweep_groups had inline (n = 64, 5 000, 10 000, 60 000), and zeros_match, which every field of the binding
taken alone must break.  They run in tests/own_slots_check.cpp, a stand-alone program built with -fsanitize=address,undefined that
checks by itself and must end clean."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rnaelem_amd", "csrc")
SRC = os.path.join(HERE, "own_slots_check.cpp")
EXE = os.path.join(HERE, "own_slots_check_asan")


def test_own_slot_sizing_mapping_and_binding():
    deps = [SRC, os.path.join(CSRC, "slot_sizing.h"), os.path.join(CSRC, "device_layout.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", EXE, SRC])
    # (the leak check, which some sandboxes cannot start, is left out: the program's vectors are freed by their destructors)
    r = subprocess.run([EXE], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    last = r.stdout.strip().split("\n")[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 70, r.stdout[-500:]
