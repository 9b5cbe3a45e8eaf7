"""The structure parser of helix_posteriors and loop_posteriors (rnaelem_amd/csrc/structure_rules.h) against its statement in
Python, api.structure_helices and api.structure_loops.  The C++ runs in tests/structure_check.cpp, a stand-alone program built with
-fsanitize=address,undefined that must also end clean; all results are integers and texts and are compared exactly."""
import itertools
import os
import random
import subprocess

import pytest

from rnaelem_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rnaelem_amd", "csrc")
SRC = os.path.join(HERE, "structure_check.cpp")
EXE = os.path.join(HERE, "structure_check_asan")

# the literal cases of test_helix_cpu.test_structure_helices and test_loop_cpu.test_structure_loops
LITERAL = ["", "....", "((...))", "((.(...)))", "(((...)).)", "(.(...)..)", ".((..))(...).", "((..)(..))", "()",
           "(.(...)..)(((..)(..)))"]
LITERAL_BAD = ["(", ")", "(()", "())", ")(", "(.x.)", "[..]"]


def balanced(n):
    """every string of length n over ( ) . whose brackets balance"""
    if n == 0:
        return [""]
    out = ["." + s for s in balanced(n - 1)]
    for inner in range(n - 1):   # ( inner ) rest
        out += ["(" + a + ")" + b for a in balanced(inner) for b in balanced(n - 2 - inner)]
    return out


def random_balanced(rng, n):
    """a balanced string of length n: brackets opened and closed at random, what stays open at the end becomes dots"""
    s, stack = [], []
    for p in range(n):
        r = rng.random()
        if r < 0.35:
            stack.append(p)
            s.append("(")
        elif r < 0.65 and stack:
            stack.pop()
            s.append(")")
        else:
            s.append(".")
    for p in stack:
        s[p] = "."
    return "".join(s)


def expected(db):
    """the line of tests/structure_check.cpp for db, from the Python statement of the rules"""
    try:
        stems, loops = api.structure_helices(db), api.structure_loops(db)
    except ValueError as e:
        return "error " + str(e)
    cols = ["ok", "S"] + [str(v) for i, j, n in stems for v in (i, j - i, n)]
    cols += ["L"] + [str(v) for t, i, j, k, l in loops for v in (t, i, j - i, k, l)]
    return " ".join(cols)


@pytest.fixture(scope="module")
def exe():
    deps = [SRC, os.path.join(CSRC, "structure_rules.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", EXE, SRC])
    return EXE


def check(exe, dbs):
    assert not any("\n" in db for db in dbs)
    # (the leak check, which some sandboxes cannot start, is left out: the program holds std::vectors and strings only)
    r = subprocess.run([exe], input="".join(db + "\n" for db in dbs), capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert len(out) == len(dbs)
    for db, got in zip(dbs, out):
        assert got == expected(db), db
    return out


def test_literal_cases_and_short_strings(exe):
    out = check(exe, LITERAL + ["()", ".", "(", ")", "x"] + LITERAL_BAD)
    assert out[0] == "ok S L" and out[LITERAL.index("()")] == "ok S 0 2 1 L 1 0 2 -1 -1"
    assert out[LITERAL.index("(.(...)..)")] == "ok S 0 10 1 2 5 1 L 4 0 10 2 7 1 2 5 -1 -1"


def test_the_three_refusals(exe):
    out = check(exe, ["..)..", "(.))", "((..)", "(", "..x..", "(a)", "[..]", ")x", "x)"])
    assert out[:4] == ["error unbalanced structure"] * 4                  # a ) that closes nothing, an unclosed (
    assert out[4:7] == ["error a structure holds ( ) . only"] * 3         # a foreign character
    assert out[7:] == ["error unbalanced structure", "error a structure holds ( ) . only"]   # the first fault in reading order decides


def test_every_balanced_string_to_length_10(exe):
    dbs = [db for n in range(11) for db in balanced(n)]
    assert len(dbs) == sum((1, 1, 2, 4, 9, 21, 51, 127, 323, 835, 2188)) and len(set(dbs)) == len(dbs)   # the Motzkin numbers
    out = check(exe, dbs)
    assert all(line.startswith("ok") for line in out)
    types = {line.split(" L")[1].split()[t] for line in out for t in range(0, len(line.split(" L")[1].split()), 5)}
    assert types == {"1", "2", "3", "4", "5"}


def test_every_string_to_length_7_balanced_or_not(exe):
    dbs = ["".join(c) for n in range(8) for c in itertools.product("().", repeat=n)]
    out = check(exe, dbs)
    assert sum(line.startswith("ok") for line in out) == sum((1, 1, 2, 4, 9, 21, 51, 127))


def test_random_balanced_strings(exe):
    rng = random.Random(20240611)
    dbs = [random_balanced(rng, rng.randint(11, 120)) for _ in range(400)]
    out = check(exe, dbs)
    assert all(line.startswith("ok") for line in out) and sum(line != "ok S L" for line in out) > 350
