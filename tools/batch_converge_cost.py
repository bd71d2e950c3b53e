#!/usr/bin/env python3
"""Cost of checking a batch of N same-size images for their fixed points, in
one launch against image by image, and of the batch loop that uses it:

    tools/batch_converge_cost.py W H {grey,rgb,rgba} N [--border B] [--filter F] [--check-every K]
                                 [--max-reps R] [--iters I] [--compact]

Image k is the synthetic random image of seed k with its values shifted right
by 0, 2, 4 or 6 bits (k mod 4): contrasts differ, so the images reach their
fixed points after different numbers of repetitions.

Prints one JSON line:
  * one batched check of the N resident images — the residual launch alone
    between two stream events (`BatchEngine.time_residual`), and
    `BatchEngine.residual(N)` timed on the host, read-back included;
  * the same number of checks made one by one through a single-image engine on
    a resident frame (`BandEngine.residual()`, host-timed per N calls; its
    launch alone between stream events, times N);
  * `run_until_stable(max_reps, K, N)` against `run(max_reps, N)`, both timed
    on the host from the enqueue to the end of the stream, uploads excluded;
  * the per-image `reps_done`, `converged` flags and the number of checks.
Every list holds all `--iters` samples; the summary fields are medians.

With `--compact` a second JSON line follows: `run_until_stable(max_reps, K, N)`
with compaction off and on, alternated in this process (one untimed pass of
each first), both loops as all samples and as min / median / max, the launches
and `image_launches` of both, and the tuned tile table."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import pconv  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("width", type=int)
    p.add_argument("height", type=int)
    p.add_argument("channels", choices=["grey", "rgb", "rgba"])
    p.add_argument("n", type=int)
    p.add_argument("--border", default="replicate", choices=["zero", "replicate"])
    p.add_argument("--filter", default="gaussian")
    p.add_argument("--check-every", type=int, default=None)
    p.add_argument("--max-reps", type=int, default=512)
    p.add_argument("--iters", type=int, default=7)
    p.add_argument("--compact", action="store_true",
                   help="also time run_until_stable with compaction off and on, alternated (a second JSON line)")
    a = p.parse_args()
    nat = pconv.native
    w, h, n = a.width, a.height, a.n
    c = {"grey": 1, "rgb": 3, "rgba": 4}[a.channels]
    fuse = nat.auto_fuse(a.filter, "auto", w * h * c, c)
    k = a.check_every or 16 * fuse
    stack = np.stack([pconv.synthetic_image(w, h, a.channels, seed=i) >> (2 * (i % 4)) for i in range(n)])
    flat = stack.reshape(-1)

    beng = nat.BatchEngine(w, h, a.channels, n, a.filter, fuse=fuse, border=a.border)
    beng.upload(flat, n)
    beng.run(k, n)  # warm: code objects, tile-shape tuning of the chunk's launches
    beng.run(a.max_reps, n)
    beng.synchronize()
    beng.upload(flat, n)
    start = beng.residual(n)
    beng.time_residual(1, n)
    batch_launch = beng.time_residual(a.iters, n)
    batch_check = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        beng.residual(n)
        batch_check.append((time.perf_counter() - t0) * 1e3)

    one = nat.BandEngine(w, h, a.channels, a.filter, 0, 1, 0, halo=fuse, fuse=fuse, border=a.border)
    one.upload(stack[0].reshape(-1), 0, h)
    one.synchronize()
    one.residual()
    one.time_residual(1)
    single_launch = one.time_residual(a.iters)
    single_checks = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        for _ in range(n):
            one.residual()
        single_checks.append((time.perf_counter() - t0) * 1e3)
    del one

    stable, fixed, infos = [], [], None
    for _ in range(a.iters):
        beng.upload(flat, n)
        beng.synchronize()
        t0 = time.perf_counter()
        infos = beng.run_until_stable(a.max_reps, k, n)
        stable.append((time.perf_counter() - t0) * 1e3)
        beng.upload(flat, n)
        beng.synchronize()
        t0 = time.perf_counter()
        beng.run(a.max_reps, n)
        beng.synchronize()
        fixed.append((time.perf_counter() - t0) * 1e3)

    def r(xs):
        return [round(x, 4) for x in xs]

    med = statistics.median
    print(json.dumps({
        "shape": f"{n} x {w}x{h} {a.channels}", "filter": a.filter, "border": a.border, "fuse": fuse,
        "check_every": k, "max_reps": a.max_reps, "residual_of_input": [int(x) for x in start],
        "batch_residual_launch_ms": r(batch_launch), "batch_check_host_ms": r(batch_check),
        "single_residual_launch_ms": r(single_launch), "n_single_checks_host_ms": r(single_checks),
        "batch_launch_median_ms": round(med(batch_launch), 4),
        "n_single_launches_median_ms": round(n * med(single_launch), 4),
        "batch_check_median_ms": round(med(batch_check), 4),
        "n_single_checks_median_ms": round(med(single_checks), 4),
        "run_until_stable_ms": r(stable), "run_max_reps_ms": r(fixed),
        "run_until_stable_median_ms": round(med(stable), 4), "run_max_reps_median_ms": round(med(fixed), 4),
        "reps_done": [int(s[0]) for s in infos], "converged": [bool(s[1]) for s in infos],
        "checks": max(int(s[3]) for s in infos),
    }))

    if not a.compact:
        return
    # Compaction off and on, alternated in this one process (one warm pass of
    # each first: a compacted launch never tunes, it runs the model's tile or
    # the tuned entry of its own image count).
    loops = {False: [], True: []}
    image_launches, launches, results = {}, {}, {}
    for it in range(a.iters + 1):
        for compact in (False, True):
            beng.upload(flat, n)
            beng.synchronize()
            t0 = time.perf_counter()
            results[compact] = beng.run_until_stable(a.max_reps, k, n, compact=compact)
            ms = (time.perf_counter() - t0) * 1e3
            if it > 0:
                loops[compact].append(ms)
            image_launches[compact] = int(beng.stats.image_launches)
            launches[compact] = int(beng.stats.launches)
    assert results[True] == results[False], "compaction changed the per-image results"

    def mmm(xs):
        return [round(min(xs), 4), round(med(xs), 4), round(max(xs), 4)]

    print(json.dumps({
        "shape": f"{n} x {w}x{h} {a.channels}", "filter": a.filter, "border": a.border, "fuse": fuse,
        "check_every": k, "max_reps": a.max_reps,
        "loop_off_ms": r(loops[False]), "loop_compact_ms": r(loops[True]),
        "loop_off_min_median_max_ms": mmm(loops[False]), "loop_compact_min_median_max_ms": mmm(loops[True]),
        "launches_off": launches[False], "launches_compact": launches[True],
        "image_launches_off": image_launches[False], "image_launches_compact": image_launches[True],
        "tuned": [[list(map(int, key)), list(map(int, shape))] for key, shape in nat.swar_tuned()],
    }))


if __name__ == "__main__":
    main()
