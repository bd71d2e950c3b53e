"""The SWAR tile-shape table and the latency model built on it, pinned to a
recording (tests/golden/swar_model.json) made without a device, where the
model answers from its resource estimate: the list of shapes in order, the
buffer-op kernel's subset, and for eight launch geometries the model's pick,
every shape's (lw, m, nw, vgpr, lds) and its predicted cycles.  Order is
behaviour (pick_swar_shape keeps the first minimum; forced buffer-op mode
falls back to the first of its shapes that runs, which must be (4, 8, 8)).

Cycles compare to a relative 1e-9: the model is a few dozen double operations,
so regrouping an expression moves the last bits and anything larger is a
changed formula.  With a device the model uses the kernels' real registers
and LDS, which the recording does not hold: the model checks skip there.
"""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swar_model.json")
REL = 1e-9


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_swar_shape_lists(native, golden):
    assert [list(s) for s in native.swar_shapes()] == golden["shapes"]
    pf = [list(s) for s in native.swar_prefetch_shapes()]
    assert pf[0] == [4, 8, 8]
    assert len(pf) == len(golden["prefetch_shapes"])
    assert sorted(pf) == sorted(golden["prefetch_shapes"])
    assert all(s in golden["shapes"] for s in pf)


def test_swar_model_matches_recording(native, golden):
    for g in golden["geometries"]:
        args = (g["steps"], g["channels"], g["rows"], g["row_bytes"])
        table = native.swar_model_table(*args)
        if any(t[5] for t in table):
            pytest.skip("a device is present: the model uses measured kernel resources")
        pick, cycles = native.swar_model(*args)
        assert list(pick) == g["pick"], args
        assert cycles == pytest.approx(g["pick_cycles"], rel=REL, abs=0), args
        assert len(table) == len(g["table"]), args
        for got, want in zip(table, g["table"]):
            assert list(got[:5]) == want[:5], (args, want[:3])
            assert got[6] == pytest.approx(want[5], rel=REL, abs=0), (args, want[:3])
