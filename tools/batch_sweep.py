#!/usr/bin/env python3
"""Image batches against one image after another, on one GPU, in one process:

    tools/batch_sweep.py [--configs 1920x630:grey,1920x630:rgb,1920x2520:rgb] [--filters gaussian,box]
                         [--batches 1,2,4,8,16,32] [--reps 40] [--iters 7] [--tune on|off]

For every configuration and B, both paths are warmed (which tunes them, with
--tune on), then timed alternately `iters` times each:

* batch:  B images through one BatchEngine — ceil(reps / fuse) launches;
* single: the same B images one after another through one Engine (the path
  before batches existed) — B x ceil(reps / fuse) launches.

Two times per path, both per image:

* loop  — hipEvents on the engine's stream around the repetitions of all B
  images, on frames already resident (the single path re-runs its resident
  frame B times between the two events: the repetitions cost the same whatever
  the bytes);
* e2e   — host clock around upload + repetitions + download of all B images
  from / to pinned host memory, ending in a synchronise.

One JSON line per (configuration, filter, B) with min / median / max of each
and the tile shape each path ran ("tuned" entries of that geometry; with
--tune off the latency model's pick)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pconv  # noqa: E402

CH = {"grey": 1, "rgb": 3, "rgba": 4}


def mmm(v):
    v = sorted(v)
    return {"min": v[0], "median": statistics.median(v), "max": v[-1]}


def event_ms(stream, work):
    """ms between two timing events recorded on `stream` around work()."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = torch.cuda.ExternalStream(stream)
    e0.record(s)
    work()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def shapes_of(n, ch, rows, row_bytes, batch, steps, model_args):
    """Tile shapes the launches of this geometry ran: the tuner's entries
    (SWAR kernels) or, untuned, the model's pick."""
    if model_args is None:
        return []  # float kernel: its tuned table is not exported
    got = [(list(k), list(s)) for k, s in n.swar_tuned()
           if k[0] == ch and k[2] == rows and k[3] == row_bytes and k[6] == batch]
    if got:
        return [{"steps": k[1], "form": k[4], "kernel": "bufop" if k[5] else "tile", "shape": s} for k, s in got]
    pick, _ = n.swar_model(steps, *model_args, batch=batch)
    return [{"steps": steps, "model_pick": list(pick)}]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="1920x630:grey,1920x630:rgb,1920x2520:rgb")
    p.add_argument("--filters", default="gaussian,box")
    p.add_argument("--batches", default="1,2,4,8,16,32")
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--iters", type=int, default=7)
    p.add_argument("--tune", choices=["on", "off"], default="on")
    a = p.parse_args()
    if a.iters < 5:
        p.error("--iters must be >= 5")
    if not torch.cuda.is_available():
        sys.exit("batch_sweep: no GPU (nothing here can be measured without one)")
    n = pconv.native
    n.set_autotune(a.tune == "on")
    for cfg in a.configs.split(","):
        size, chn = cfg.split(":")
        w, h = (int(x) for x in size.split("x"))
        c = CH[chn]
        for filt in a.filters.split(","):
            single = pconv.Engine(w, h, chn, filt)
            fuse = single.fuse
            for B in (int(b) for b in a.batches.split(",")):
                batch = pconv.BatchEngine(w, h, chn, B, filt, fuse=fuse)
                nbytes = w * h * c
                pin_in, pin_out = n.PinnedBuffer(B * nbytes), n.PinnedBuffer(B * nbytes)
                host_in = np.frombuffer(pin_in, dtype=np.uint8)
                for b in range(B):
                    host_in[b * nbytes:(b + 1) * nbytes] = pconv.synthetic_image(w, h, chn, seed=b + 1).reshape(-1)
                be, se = batch._eng, single._eng

                def batch_loop():
                    return event_ms(be.compute_stream, lambda: be.run(a.reps, B))

                def single_loop():
                    def work():
                        for _ in range(B):
                            se.run(a.reps)
                    return event_ms(se.compute_stream, work)

                def batch_e2e():
                    t0 = time.perf_counter()
                    be.upload_ptr(pin_in.ptr, B)
                    be.run(a.reps, B)
                    be.download_ptr(pin_out.ptr, B)
                    be.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                def single_e2e():
                    t0 = time.perf_counter()
                    for b in range(B):
                        se.upload_ptr(pin_in.ptr + b * nbytes, w * c, 0, h)
                        se.run(a.reps)
                        se.download_ptr(pin_out.ptr + b * nbytes, w * c, 0, h)
                    se.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                # warm both paths: code objects, tuning, copy set-up; and the
                # two give the same bytes
                single_e2e()
                ref = np.frombuffer(pin_out, dtype=np.uint8).copy()
                batch_e2e()
                if not np.array_equal(ref, np.frombuffer(pin_out, dtype=np.uint8)):
                    sys.exit(f"batch_sweep: batch and single results differ ({cfg} {filt} B={B})")
                batch_loop(), single_loop()
                t = {"batch_loop": [], "single_loop": [], "batch_e2e": [], "single_e2e": []}
                for _ in range(a.iters):
                    t["batch_loop"].append(batch_loop())
                    t["single_loop"].append(single_loop())
                for _ in range(a.iters):
                    t["batch_e2e"].append(batch_e2e())
                    t["single_e2e"].append(single_e2e())
                margs = (chn, h, w * c) if filt == "gaussian" else None
                steps = min(fuse, a.reps)
                out = {"width": w, "height": h, "channels": chn, "filter": filt, "reps": a.reps, "fuse": fuse,
                       "batch": B, "iters": a.iters, "tune": a.tune,
                       "launches": {"batch": be.stats.launches, "single": B * se.stats.launches},
                       "shapes": {"batch": shapes_of(n, c, h, w * c, B, steps, margs),
                                  "single": shapes_of(n, c, h, w * c, 1, steps, margs)}}
                for k, v in t.items():  # ms per image
                    out[k + "_ms_per_image"] = mmm([x / B for x in v])
                print(json.dumps(out), flush=True)
                del batch, be, pin_in, pin_out, host_in
            del single, se


if __name__ == "__main__":
    main()
