"""CPU: the ordering of consecutive pipelined batches (csrc/imt_apply_pipe.hpp, the rule imt_itree.cpp takes its stream
waits from) against a model of what every launch reads and writes (tests/native/apply_pipe_sched.cpp).

Exhaustive over every depth <= 6, every kind (apply / witness) and every occupied height l0 of every batch of every chain
of two and of three batches: each pair of launches of different batches that conflict on a stored level (read after write,
write after read, write after write) must be ordered by stream order plus the header's waits.  Chains of three test that
waiting for the batch directly in front is enough (transitivity).

A checker that accepts everything shows nothing, so the same checker must find the hazard in the one-level spacing of the
witness pipeline when it is used for apply behind apply (the launch that writes level l of the batch behind starting as
soon as the batch in front has written level l, while its next launch still reads it), and in no waits at all."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "indexed-merkle-tree-halo2_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "apply_pipe_sched.cpp")
GXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out[key] = rest
    return out


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("applypipe") / "apply_pipe_sched")
    subprocess.run(GXX + ["-O2", "-o", exe, SRC], check=True)
    return run(exe)


def test_every_conflict_is_ordered(report):
    assert int(report["rule_hazards"]) == 0, report.get("first_hazard")
    # depth d has 2d batches: (2d)^2 pairs and (2d)^3 triples, d = 1 .. 6
    assert int(report["rule_cases"]) == sum((2 * d) ** 2 + (2 * d) ** 3 for d in range(1, 7))


def test_the_checker_sees_the_one_level_spacing(report):
    assert int(report["spaced1_hazards"]) > 0
    # the smallest case already shows it: the chain of the batch in front reads level 0 while the one behind writes it
    assert "depth 1" in report["first_spaced1_hazard"]


def test_the_checker_sees_no_order_at_all(report):
    assert int(report["unordered_hazards"]) > int(report["spaced1_hazards"])


def test_the_checker_under_sanitizers(tmp_path):
    exe = str(tmp_path / "apply_pipe_sched_san")
    subprocess.run(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    assert int(run(exe)["rule_hazards"]) == 0
