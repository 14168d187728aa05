"""Every way a batch goes through api.cpp's runners, one call each (tests/call_shapes.py), pinned against the PARENT
commit's library: the launches and units per profile family and the multi-adapter path of every call equal the record in
tests/golden/call_shapes.json (tests/golden/make_call_shapes_golden.py, run once on the parent's build, never on the code
under test), and every call's results equal the oracle's -- a memset of the wrong size or in the wrong place is a wrong row
or status byte, not a count.  GPU only."""
import json
import os

import numpy as np
import pytest

import call_shapes

pytestmark = pytest.mark.gpu

SHAPES = call_shapes.shapes()
_expected = {}


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(os.path.dirname(__file__), "golden", "call_shapes.json")) as fh:
        return json.load(fh)["shapes"]


def test_the_fixture_names_every_shape(fixture):
    assert sorted(fixture) == sorted(s.name for s in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_call_shape(hip, orc, fixture, shape):
    record, results = call_shapes.run(shape)
    parent = fixture[shape.name]
    print(shape.name, "this", record, "parent", parent)
    assert record == parent
    # the path the shape was chosen for -- of the parent's call and of this one; a uniform batch of one adapter makes ONE prefilter pass
    assert record["path"] == shape.path
    if shape.kind == "uniform" and len(shape.ads) == 1 and shape.ads[0].matcher_spec().kmer_sets is not None \
            and shape.name != "anchored exact":
        assert parent["launches"][0] == 1 and parent["units"][0] == shape.n
    key = (shape.reads_of, shape.kind, shape.n)
    if key not in _expected:
        _expected[key] = call_shapes.expected(orc, shape)
    locate = shape.kind in ("locate", "host_locate")
    for i, ((g6, gst, gbest), (w6, wst, wbest)) in enumerate(zip(results, _expected[key])):
        if shape.kind == "linked" and i == 2:            # the views: starts and lengths
            assert np.array_equal(g6, w6) and np.array_equal(gst, wst), (shape.name, "views")
            continue
        assert np.array_equal(gst, wst), (shape.name, i, np.nonzero(gst != wst)[0][:5])
        if w6 is None:
            continue
        f = wst == 1
        # (Aligner.locate over a batch writes the rows of the reads it finds; the match calls clear the others)
        bad = np.nonzero(((g6 != w6).any(axis=1)) & (f if locate else True))[0]
        assert len(bad) == 0, (shape.name, i, bad[:5], g6[bad[:3]], w6[bad[:3]])
        if gbest is not None and wbest is not None:
            assert np.array_equal(gbest[f], wbest[f]), (shape.name, i)
            if not locate:
                assert (gbest[~f] == -1).all(), (shape.name, i, "best adapter of reads without a match")
