"""CPU test of the lockstep walks' successor rule (restir-embree_amd/csrc/rs_lockstep.h lockstep_next, the function
occluded_wave_multi / occluded_wave / closest_wave call for the wave's next node).

tests/cpp/lockstep_successor.cpp runs the wave automaton on random preorder skip trees (1-300 nodes; random, chain
and full shapes; a single-leaf root), 1-128 rays, hit / miss / ended-at-leaf decided by a hash of (ray, node) with
ending probabilities 0, 0.5 and 1, some or all rays inactive from the start -- once with the exact minimum of the
cursors at every step and once with the rule.  It fails unless the visited-node sequences and every ray's outcome are
equal, the rule's answer is the minimum at every step, and the reduce sentinel comes back exactly on the leaf steps
where every ray on the node ended."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lockstep_successor.cpp")
HDR = os.path.join(ROOT, "restir-embree_amd", "csrc", "rs_lockstep.h")
EXE = os.path.join(ROOT, "oracle", "_build", "lockstep_successor")


def _exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", EXE, SRC])
    return EXE


def test_successor_rule_equals_exact_minimum():
    p = subprocess.run([_exe()], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.match(r"ok cases=(\d+) steps=(\d+) descend=(\d+) interior_skip=(\d+) leaf=(\d+) reductions=(\d+)", p.stdout)
    assert m, p.stdout
    cases, steps, descend, interior_skip, leaf, reductions = map(int, m.groups())
    assert cases == 3 * 40 * 3 * 4 * 3
    # every kind of step was exercised, the reduction among them
    assert min(descend, interior_skip, leaf, reductions) > 100 and descend + interior_skip + leaf == steps
