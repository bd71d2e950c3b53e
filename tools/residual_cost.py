#!/usr/bin/env python3
"""Cost of one convergence check next to one fused launch of the production
kernel, on the same frame in the same process:

    tools/residual_cost.py W H {grey,rgb,rgba} [--filter F] [--border B] [--fuse T] [--iters N]

The frame holds a synthetic random image.  One fused launch is
`BandEngine.run(fuse)` (its hipEvent `loop_ms`, after a warm run that also
tunes the tile shape); one check is the residual kernel alone between two
timing events on the same stream (`BandEngine.time_residual`, after a warm
launch).  Prints one JSON line with every timed launch and the minima.  A
check reads the frame once, a fused launch reads and writes it: the check
should take no longer."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pconv  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("width", type=int)
    p.add_argument("height", type=int)
    p.add_argument("channels", choices=["grey", "rgb", "rgba"])
    p.add_argument("--filter", default="gaussian")
    p.add_argument("--border", default="zero", choices=["zero", "replicate"])
    p.add_argument("--fuse", type=int, default=None)
    p.add_argument("--iters", type=int, default=7)
    a = p.parse_args()
    n = pconv.native
    w, h = a.width, a.height
    c = {"grey": 1, "rgb": 3, "rgba": 4}[a.channels]
    fuse = a.fuse or n.auto_fuse(a.filter, "auto", w * h * c, c)
    eng = n.BandEngine(w, h, a.channels, a.filter, 0, 1, 0, halo=fuse, fuse=fuse, border=a.border)
    rows = min(h, 4096)  # upload in slabs: no second copy of a large image on the host
    buf = np.empty(rows * w * c, np.uint8)
    for y in range(0, h, rows):
        k = min(rows, h - y)
        n.synth_rows(buf, w, h, a.channels, 1, y, k)
        eng.upload(buf[: k * w * c], y, y + k)
    eng.synchronize()
    start = eng.residual()
    eng.run(fuse)  # warm: code object, tile-shape tuning
    eng.synchronize()
    fused = []
    for _ in range(a.iters):
        eng.run(fuse)
        eng.synchronize()
        assert eng.stats.launches == 1
        fused.append(eng.stats.loop_ms)
    eng.time_residual(1)
    check = eng.time_residual(a.iters)
    print(json.dumps({
        "shape": f"{w}x{h} {a.channels}", "filter": a.filter, "border": a.border, "fuse": eng.fuse,
        "frame_bytes": w * h * c, "residual_of_input": start,
        "fused_launch_ms": [round(x, 4) for x in fused], "residual_launch_ms": [round(x, 4) for x in check],
        "fused_min_ms": round(min(fused), 4), "residual_min_ms": round(min(check), 4),
        "residual_gb_per_s": round(w * h * c / min(check) / 1e6, 1),
    }))


if __name__ == "__main__":
    main()
