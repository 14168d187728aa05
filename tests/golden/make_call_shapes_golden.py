"""Record tests/golden/call_shapes.json: the launches and units per profile family and the multi-adapter path of every call
shape of tests/call_shapes.py, on the library of the commit BEFORE a host-side change to api.cpp's runners.

    CAH_LIB_PATH=/path/to/the/parent/build/libcutadapt_hip.so python tests/golden/make_call_shapes_golden.py [--out FILE]

Needs the GPU.  CAH_LIB_PATH must be set: the fixture is what the code under test is compared WITH and is never regenerated
from it.  --check also compares every call's results with the oracle (that the shapes themselves are sound)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "call_shapes.json"))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    assert os.environ.get("CAH_LIB_PATH"), "CAH_LIB_PATH: the parent commit's build of the library"
    import call_shapes
    from cutadapt_amd import _lib
    doc = {"library_build_id": _lib.build_id(), "families": ["filter", "dp", "comparer", "scan", "merge"], "shapes": {}}
    for shape in call_shapes.shapes():
        record, results = call_shapes.run(shape)
        assert record["path"] == shape.path, (shape.name, record)
        doc["shapes"][shape.name] = record
        print(shape.name, json.dumps(record), flush=True)
        if a.check:
            import numpy as np
            from oracle import oracle
            oracle.build()
            for (g6, gst, _), (w6, wst, _) in zip(results, call_shapes.expected(oracle, shape)):
                if w6 is not None and w6.ndim == 1:                    # a linked call's views: starts and lengths
                    assert np.array_equal(g6, w6) and np.array_equal(gst, wst), shape.name
                    continue
                assert np.array_equal(gst, wst), shape.name
                if w6 is not None:
                    assert np.array_equal(g6[wst == 1], w6[wst == 1]), shape.name
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
