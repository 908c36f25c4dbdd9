"""The training walk of the glancer's MobileNetV2 (adafocus_amd/glancer_train.py) makes, launch for launch, the C-ABI calls it made when it
stated its own conv + BatchNorm layer treatment, before that moved into the core it shares with the trunk (adafocus_amd/layer_train.py):
tests/golden/glancer_walk_launches.json holds, per case of tools/glancer_walk_launches.py, the sha256 of the sorted launch lines (symbol,
scalars, ConvParams, every tensor operand named by what produced it) and the launch count per symbol, recorded from that code and never
regenerated from the code under test.  No GPU: the replacements of tools/trunk_walk_launches.py.  This is what holds the skipping rules --
no BatchNorm backward, weight-gradient, data-gradient or `add` launch appears or disappears for any pattern of requires_grad -- and the
operands of every launch; the order of independent launches is free.  On a mismatch: `python tools/glancer_walk_launches.py --dump CASE`
here and at the recorded commit, and diff."""
import json
import os

import pytest

from tests.helpers import GOLDEN, load_tool

W = load_tool("glancer_walk_launches")

with open(os.path.join(GOLDEN, "glancer_walk_launches.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recording_covers_the_case_list():
    assert set(RECORDED["cases"]) == set(W.CASES)
    assert set(W.CASES) == {"all", "tail", "bn_affine", "mid_dw", "res_project", "stem", "none"}


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
