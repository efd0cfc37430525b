"""GPU test of the sweep's plans against the plans the library made before planning moved into mc33_sweep_plan.h
(tests/golden/sweep_plans.json, recorded by tools/record_sweep_plans.py): the sequences of tests/sweep_plan_sequences.py are
replayed, and after every step the plan in force - every tile in launch order, the tile count, the plan bit and the plane weight -
is the recorded one.  There is no tolerance in this file.

A plan depends on the blocks the device holds at once.  A sequence whose recorded plans were made for another number of
resident blocks than this device reports is skipped, and says so; on a device like the one the file was recorded on (256
compute units) nothing is skipped."""
import json
import os

import pytest

import sweep_plan_sequences as sq

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEQUENCES = {s[0]: s for s in sq.sequences()}
_fields = {}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "sweep_plans.json")) as f:
        g = json.load(f)
    assert sorted(s["name"] for s in g["sequences"]) == sorted(SEQUENCES), "the recorded sequences are not the ones of sweep_plan_sequences.py"
    return g


def field(shape):
    import torch
    if shape not in _fields:
        _fields[shape] = torch.from_numpy(sq.field_of(shape)).cuda()
    return _fields[shape]


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_plans_are_the_recorded_ones(golden, name):
    rec = next(s for s in golden["sequences"] if s["name"] == name)
    seq = SEQUENCES[name]
    assert rec["env"] == seq[2] and len(rec["steps"]) == len(seq[3]), "recorded under another environment, or with other steps"
    got = sq.replay(seq, field(seq[1]))
    for step, (g, at) in enumerate(zip(got, rec["steps"])):
        want = golden["plans"][at]
        if g["info"][1] != want["info"][1]:
            pytest.skip("%s: this device holds %d sweep blocks at once, the plans were recorded at %d" % (name, g["info"][1], want["info"][1]))
        assert g["info"] == want["info"] and g["weight"] == want["weight"], (name, step, g["info"], want["info"], g["weight"], want["weight"])
        assert g["tiles"] == want["tiles"], (name, step, "tiles differ", next(k // 4 for k in range(len(g["tiles"])) if g["tiles"][k] != want["tiles"][k]))
