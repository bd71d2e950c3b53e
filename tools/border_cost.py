#!/usr/bin/env python3
"""Device-resident loop time (hipEvent `loop_ms` of BandEngine.run) of the
zero and the replicate border on one geometry, interleaved run by run:

    tools/border_cost.py W H {grey,rgb,rgba} REPS [--fuse T] [--iters N] [--borders zero,replicate]

Both engines share the process, so the tile shape tuned for the geometry by
the first one is the shape the other runs too (the tuned-shape cache is keyed
on the geometry, not on the border).  Prints one JSON line: min / median / max
of the loop in ms and in us per repetition, per border, and the tuned shapes.
Only tiles that touch an image edge do extra work under replicate; a gap well
beyond those tiles' share means the correction runs in interior tiles."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pconv  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("width", type=int)
    p.add_argument("height", type=int)
    p.add_argument("channels", choices=["grey", "rgb", "rgba"])
    p.add_argument("reps", type=int)
    p.add_argument("--filter", default="gaussian")
    p.add_argument("--fuse", type=int, default=None)
    p.add_argument("--iters", type=int, default=7)
    p.add_argument("--borders", default="zero,replicate")
    a = p.parse_args()
    borders = a.borders.split(",")
    img = np.ascontiguousarray(pconv.synthetic_image(a.width, a.height, a.channels, seed=1)).reshape(-1)
    engs = {}
    for b in borders:
        e = pconv.Engine(a.width, a.height, a.channels, a.filter, fuse=a.fuse, border=b)
        e._eng.upload(img, 0, a.height)
        e._eng.run(a.reps)  # tunes (first engine), loads the code objects
        e._eng.synchronize()
        engs[b] = e
    ms = {b: [] for b in borders}
    for _ in range(a.iters):
        for b in borders:
            engs[b]._eng.run(a.reps)
            engs[b]._eng.synchronize()
            ms[b].append(engs[b].stats.loop_ms)
    out = {"width": a.width, "height": a.height, "channels": a.channels, "reps": a.reps, "filter": a.filter,
           "fuse": engs[borders[0]].fuse, "iters": a.iters, "tuned": [list(map(list, t)) for t in pconv.native.swar_tuned()]}
    for b in borders:
        v = sorted(ms[b])
        out[b] = {"loop_ms": {"min": v[0], "median": statistics.median(v), "max": v[-1]},
                  "us_per_rep": {"min": 1e3 * v[0] / a.reps, "median": 1e3 * statistics.median(v) / a.reps,
                                 "max": 1e3 * v[-1] / a.reps}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
