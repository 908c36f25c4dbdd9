"""The training walk of the ResNet trunk (adafocus_amd/trunk_train.py) makes, launch for launch, the C-ABI calls the two walks made before
they were merged into one: tests/golden/trunk_walk_launches.json holds, per case of tools/trunk_walk_launches.py, the sha256 of the sorted
launch lines (symbol, scalars, ConvParams, every tensor operand named by what produced it) and the launch count per symbol, recorded from
that code and never regenerated from the code under test.  No GPU: hip_ops._call, hip_ops._workspace and _lib.need_gpu_f32 are replaced for
the duration of a test and the wrappers run their shape logic on CPU tensors.  This is what holds the skipping rules -- no relu_backward,
weight-gradient, data-gradient or shift launch appears or disappears for any pattern of requires_grad -- and the operands of every launch;
the order of independent launches is free.  On a mismatch: `python tools/trunk_walk_launches.py --dump CASE` here and at the recorded
commit, and diff."""
import json
import os

import pytest

from tests.helpers import GOLDEN, load_tool

W = load_tool("trunk_walk_launches")

with open(os.path.join(GOLDEN, "trunk_walk_launches.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recording_covers_the_case_list():
    assert set(RECORDED["cases"]) == set(W.CASES)
    assert len(W.CASES) == 2 * 3 * 6 + 2


@pytest.mark.parametrize("case", list(W.CASES))
def test_launches_equal_the_recorded_walk(monkeypatch, case):
    net, x4, dfeat, want, rec = W.prepare(case)
    for obj, name, value in rec.patches():
        monkeypatch.setattr(obj, name, value)
    got = W.run(net, x4, dfeat)
    assert got == want, sorted(got ^ want)              # exactly the parameters that require a gradient received one
    s = W.summary(rec)
    assert s["counts"] == RECORDED["cases"][case]["counts"], case
    assert s["digest"] == RECORDED["cases"][case]["digest"], case
