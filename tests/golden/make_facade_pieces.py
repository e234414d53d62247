"""Writes tests/golden/facade_pieces_v1.json: the calls generate_fast makes on its engine (priming, pieces, draw-ahead uploads, slices of `forced`) over
the grid of tests/facade_schedule_lib.py, recorded on a fake engine at the commit BEFORE the schedule moved into mi355_wavenet/generation.py.  Run it
only to record a deliberate change of the pieces:  python tests/golden/make_facade_pieces.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "pytorch-wavenet_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import facade_schedule_lib as fsl  # noqa: E402


class _Patch:
    setattr = staticmethod(setattr)


if __name__ == "__main__":
    model, fake = fsl.install(_Patch)
    out = os.path.join(HERE, fsl.FIXTURE)
    with open(out, "w") as f:
        json.dump(fsl.record_pieces(model, fake), f, indent=0, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")
