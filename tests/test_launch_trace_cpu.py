"""The host side of every forward / training step launches exactly what it launched before the executors were split by layer kind: the launch
trace (tests/launch_trace.py) of every scenario -- each one a branch of ``Plan.forward`` / ``Plan.backward`` / ``ResNetPlan`` / ``BNPlan`` -- equals the
one recorded in launch_trace_cpu.json, which was written from a checkout of the commit before that refactor:

    python tests/launch_trace.py --root <checkout of the parent commit> --write tests/launch_trace_cpu.json

The ``bn_train_*`` scenarios, ``resnet_forward_twice`` and the ``resnet_*_no_BN_STATS_IN_CONV`` / ``resnet_train_no_WGRAD_STREAM`` scenarios were added
to the file in the same way from commit cff3529 ("Add BatchNorm variant of YOLOv1"), the parent of the refactor that gave the two conv -> BatchNorm
executors one unit record, packer, walk and backward helper (yolo/conv_bn.py); that recording left every older entry as it was.  A trace depends on
the launch plans that earlier scenarios of the same process entered into the process-wide table, so the file is recorded, and compared, over whole runs.

A kernel change that moves launches on purpose regenerates the file from its own tree and says so."""

import json
import os
import tempfile

import pytest

import launch_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_trace_cpu.json")) as _f:
    WANT = json.load(_f)


def test_every_scenario_has_a_recorded_trace():
    assert sorted(WANT) == sorted(launch_trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(launch_trace.SCENARIOS))
def test_launch_trace_is_the_recorded_one(name):
    lines = launch_trace.SCENARIOS[name]()
    got = launch_trace.digest(lines)
    if got != WANT[name]:
        fd, path = tempfile.mkstemp(prefix=f"launch_trace_{name}_", suffix=".txt")
        with os.fdopen(fd, "w") as f:
            f.write("\n".join(lines) + "\n")
        per = [(got["lines"][i: i + 6], WANT[name]["lines"][i: i + 6]) for i in range(0, max(len(got["lines"]), len(WANT[name]["lines"])), 6)]
        first = next((i for i, (a, b) in enumerate(per) if a != b), None)
        print(f"{name}: {got['calls']} calls, recorded {WANT[name]['calls']}; full trace in {path}")
        print(f"first differing line: {first + 1}: " + (lines[first] if first < len(lines) else "(missing)"))
        print("compare with the trace of the recorded commit: python tests/launch_trace.py --root <its checkout> --dump <dir> " + name)
    assert got == WANT[name]
