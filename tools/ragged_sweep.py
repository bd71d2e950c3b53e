#!/usr/bin/env python3
"""Images of different sizes: mixed-size batches against one engine per image
and against a uniform batch of envelope-size images, on one GPU, in one process:

    tools/ragged_sweep.py [--envelope 640x480:rgb] [--n 64] [--filters gaussian,box] [--reps 40]
                          [--iters 7] [--seed 1] [--tune on|off] [--min-fill 0.5]

N synthetic images with width and height drawn uniformly from [W/2, W] and
[H/2, H] (a quarter of the envelope's area up to all of it; fixed seed).  Four
paths, each warmed (which tunes it, with --tune on), then timed alternately
`iters` times:

* many:       the size buckets of ``convolve_many`` (``size_buckets`` with
              --min-fill), one mixed-size BatchEngine run per bucket;
* one_bucket: all N in ONE mixed-size BatchEngine of the envelope;
* single:     one Engine per image, one image after another (the path before
              mixed sizes);
* uniform:    N images all AT the envelope size through a uniform BatchEngine —
              against one_bucket it shows what the extents table and the
              workgroups that leave early cost or save on the same grid.

Two times per path, both per image (as tools/batch_sweep.py):

* loop — hipEvents on the engine's stream around the repetitions on frames
  already resident (summed over a path's engines);
* e2e  — host clock around upload + repetitions + download from / to pinned
  host memory, ending in a synchronise (the single path synchronises after
  every image: its engines have a stream each).

One JSON line per filter with min / median / max of each."""
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = torch.cuda.ExternalStream(stream)
    e0.record(s)
    work()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envelope", default="640x480:rgb")
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--filters", default="gaussian,box")
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--iters", type=int, default=7)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--tune", choices=["on", "off"], default="on")
    p.add_argument("--min-fill", type=float, default=0.5)
    a = p.parse_args()
    if a.iters < 5:
        p.error("--iters must be >= 5")
    if not torch.cuda.is_available():
        sys.exit("ragged_sweep: no GPU (nothing here can be measured without one)")
    n = pconv.native
    n.set_autotune(a.tune == "on")
    size, chn = a.envelope.split(":")
    W, H = (int(x) for x in size.split("x"))
    c, N = CH[chn], a.n
    rng = np.random.default_rng(a.seed)
    sizes = [(int(w), int(h)) for w, h in zip(rng.integers((W + 1) // 2, W + 1, N), rng.integers((H + 1) // 2, H + 1, N))]
    imgs = [pconv.synthetic_image(w, h, chn, seed=k + 1) for k, (w, h) in enumerate(sizes)]
    nbytes = [w * h * c for w, h in sizes]
    total = sum(nbytes)
    for filt in a.filters.split(","):
        fuse = pconv.Engine(W, H, chn, filt).fuse
        buckets = pconv.size_buckets(sizes, chn, fuse, min_fill=a.min_fill)
        # pinned packings: per bucket (many), all N (one_bucket, single), N envelope-size images (uniform)
        pins = []

        def packed(idx):
            pin_in, pin_out = n.PinnedBuffer(sum(nbytes[i] for i in idx)), n.PinnedBuffer(sum(nbytes[i] for i in idx))
            pins.append((pin_in, pin_out))
            host, at = np.frombuffer(pin_in, dtype=np.uint8), 0
            for i in idx:
                host[at:at + nbytes[i]] = imgs[i].reshape(-1)
                at += nbytes[i]
            return pin_in, pin_out

        many = [(pconv.BatchEngine(w, h, chn, len(idx), filt, fuse=fuse)._eng, [sizes[i] for i in idx], *packed(idx))
                for (w, h), idx in buckets]
        one = [(pconv.BatchEngine(W, H, chn, N, filt, fuse=fuse)._eng, sizes, *packed(range(N)))]
        singles = [pconv.Engine(w, h, chn, filt, fuse=fuse)._eng for w, h in sizes]
        s_in, s_out = packed(range(N))
        uni = pconv.BatchEngine(W, H, chn, N, filt, fuse=fuse)._eng
        u_in, u_out = n.PinnedBuffer(N * W * H * c), n.PinnedBuffer(N * W * H * c)
        np.frombuffer(u_in, dtype=np.uint8)[:] = np.concatenate(
            [pconv.synthetic_image(W, H, chn, seed=k + 1).reshape(-1) for k in range(N)])

        def mixed_e2e(engs):
            t0 = time.perf_counter()
            for e, sz, pin_in, pin_out in engs:
                e.upload_sized_ptr(pin_in.ptr, sz)
                e.run(a.reps, len(sz))
                e.download_sized_ptr(pin_out.ptr)
            for e, *_ in engs:
                e.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def mixed_loop(engs):
            return sum(event_ms(e.compute_stream, lambda e=e, sz=sz: e.run(a.reps, len(sz))) for e, sz, *_ in engs)

        def single_e2e():
            t0, at = time.perf_counter(), 0
            for e, (w, h), k in zip(singles, sizes, nbytes):
                e.upload_ptr(s_in.ptr + at, w * c, 0, h)
                e.run(a.reps)
                e.download_ptr(s_out.ptr + at, w * c, 0, h)
                e.synchronize()
                at += k
            return (time.perf_counter() - t0) * 1e3

        def single_loop():
            return sum(event_ms(e.compute_stream, lambda e=e: e.run(a.reps)) for e in singles)

        def uniform_e2e():
            t0 = time.perf_counter()
            uni.upload_ptr(u_in.ptr, N)
            uni.run(a.reps, N)
            uni.download_ptr(u_out.ptr, N)
            uni.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def uniform_loop():
            return event_ms(uni.compute_stream, lambda: uni.run(a.reps, N))

        # warm every path (code objects, tuning, copy set-up); the three
        # mixed-size paths give the same bytes
        single_e2e()
        ref = np.frombuffer(s_out, dtype=np.uint8).copy()
        mixed_e2e(one)
        if not np.array_equal(ref, np.frombuffer(one[0][3], dtype=np.uint8)):
            sys.exit(f"ragged_sweep: one_bucket and single results differ ({filt})")
        mixed_e2e(many)
        got = np.empty_like(ref)
        offs = np.concatenate([[0], np.cumsum(nbytes)])
        for (_, idx), (_, _, _, pin_out) in zip(buckets, many):
            host, at = np.frombuffer(pin_out, dtype=np.uint8), 0
            for i in idx:
                got[offs[i]:offs[i + 1]] = host[at:at + nbytes[i]]
                at += nbytes[i]
        if not np.array_equal(ref, got):
            sys.exit(f"ragged_sweep: many and single results differ ({filt})")
        uniform_e2e()
        mixed_loop(many), mixed_loop(one), single_loop(), uniform_loop()
        t = {k: [] for k in ("many_loop", "one_bucket_loop", "single_loop", "uniform_loop", "many_e2e",
                             "one_bucket_e2e", "single_e2e", "uniform_e2e")}
        for _ in range(a.iters):
            t["many_loop"].append(mixed_loop(many))
            t["one_bucket_loop"].append(mixed_loop(one))
            t["single_loop"].append(single_loop())
            t["uniform_loop"].append(uniform_loop())
        for _ in range(a.iters):
            t["many_e2e"].append(mixed_e2e(many))
            t["one_bucket_e2e"].append(mixed_e2e(one))
            t["single_e2e"].append(single_e2e())
            t["uniform_e2e"].append(uniform_e2e())
        out = {"envelope": [W, H], "channels": chn, "filter": filt, "n": N, "seed": a.seed, "reps": a.reps, "fuse": fuse,
               "iters": a.iters, "tune": a.tune, "min_fill": a.min_fill,
               "fill_of_envelope": total / (N * W * H * c),
               "buckets": [{"envelope": [w, h], "n": len(idx),
                            "fill": sum(nbytes[i] for i in idx) / (len(idx) * w * h * c)} for (w, h), idx in buckets],
               "launches": {"many": sum(e.stats.launches for e, *_ in many), "one_bucket": one[0][0].stats.launches,
                            "single": sum(e.stats.launches for e in singles), "uniform": uni.stats.launches}}
        for k, v in t.items():  # ms per image
            out[k + "_ms_per_image"] = mmm([x / N for x in v])
        print(json.dumps(out), flush=True)
        del many, one, singles, uni, pins, s_in, s_out, u_in, u_out


if __name__ == "__main__":
    main()
