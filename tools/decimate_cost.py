#!/usr/bin/env python3
"""Cost of decimated results (docs/PERFORMANCE.md 3.8), on the GPU.

1. k_decimate alone between stream events (native.launch_decimate(timed=...))
   on an engine-like pitched frame, beside the host-timed full-size D2H of the
   same frame that a decimated download replaces (pinned host memory, same
   session): 1920x2520 rgb at s = 2 and 4, 32768^2 grey at s = 2, and a batch
   of 64 320x240 rgb frames at s = 2.
2. Engine.run_numpy of the headline image, 40 repetitions, with decimate=2
   against convolve(img, 40)[::2, ::2] (the undecimated path, which this
   feature leaves untouched), alternating, host clock around whole calls.
3. A 1920x2520 rgb pyramid to the top against the same levels from convolve
   calls with host slicing in between.

Prints one JSON line per measurement.  Needs a GPU: there is no fallback.
"""
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


def _ceil(a, b):
    return -(-a // b)


def _summary(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4),
            "n": len(xs)}


def kernel_alone(name, w, h, pb, s, frames, launches, copies):
    n = pconv.native
    rb = w * pb
    pitch = _ceil(16 + rb + 32, 128) * 128
    stride = (h + 2) * pitch
    src = torch.randint(0, 256, (frames * stride,), dtype=torch.uint8, device="cuda")
    ow, oh = _ceil(w, s), _ceil(h, s)
    dst_pitch = _ceil(ow * pb, 16) * 16
    dst_stride = oh * dst_pitch
    dst = torch.empty(frames * dst_stride, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (src.data_ptr() + pitch + 16, pitch, rb, h, dst.data_ptr(), dst_pitch, frames * dst_stride, pb, s)
    kw = dict(frames=frames, src_stride=stride, dst_stride=dst_stride, stream=stream)
    n.launch_decimate(*args, **kw, timed=5)  # warm-up: code object, caches
    ms = n.launch_decimate(*args, **kw, timed=launches)
    # what a decimated download replaces: the engine's full-size pitched D2H into pinned memory, and the
    # decimated download itself (the kernel + the D2H of the kept bytes); host clock around call + synchronise
    ch = {1: "grey", 3: "rgb", 4: "rgba"}[pb]
    full = torch.empty(frames * h * rb, dtype=torch.uint8).pin_memory()
    small = torch.empty(frames * oh * ow * pb, dtype=torch.uint8).pin_memory()
    if frames == 1:
        e = n.BandEngine(w, h, ch, "gaussian", 0, 1, 0, halo=1, fuse=1)
        plain = lambda: e.download_ptr(full.data_ptr(), rb, 0, h)  # noqa: E731
        decim = lambda: e.download_decimated_ptr(small.data_ptr(), ow * pb, s)  # noqa: E731
    else:
        e = n.BatchEngine(w, h, ch, frames, "gaussian", 0, fuse=1)
        plain = lambda: e.download_ptr(full.data_ptr(), frames)  # noqa: E731
        decim = lambda: e.download_decimated_ptr(small.data_ptr(), frames, s)  # noqa: E731

    def host_timed(call):
        t = []
        for i in range(copies + 3):
            e.synchronize()
            t0 = time.perf_counter()
            call()
            e.synchronize()
            if i >= 3:
                t.append((time.perf_counter() - t0) * 1e3)
        return t

    t_full, t_small = host_timed(plain), host_timed(decim)
    del e
    print(json.dumps({"what": "k_decimate", "case": name, "factor": s, "frames": frames, "out_bytes": frames * oh * ow * pb,
                      "in_bytes": frames * h * rb, "kernel": _summary(ms),
                      "download_full": _summary(t_full), "download_decimated": _summary(t_small)}), flush=True)


def engine_end_to_end(rounds):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(2520, 1920, 3), dtype=np.uint8)
    eng = pconv.Engine(1920, 2520, "rgb")
    for _ in range(3):
        a = eng.run_numpy(img, 40)[::2, ::2]
        b = eng.run_numpy(img, 40, decimate=2)
    assert np.array_equal(a, b)
    full, sliced, dec = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = eng.run_numpy(img, 40)
        t1 = time.perf_counter()
        out = np.ascontiguousarray(out[::2, ::2])
        t2 = time.perf_counter()
        eng.run_numpy(img, 40, decimate=2)
        t3 = time.perf_counter()
        full.append((t1 - t0) * 1e3)
        sliced.append((t2 - t0) * 1e3)
        dec.append((t3 - t2) * 1e3)
    print(json.dumps({"what": "Engine.run_numpy 1920x2520 rgb x40", "full_download": _summary(full),
                      "full_download_plus_host_slice": _summary(sliced), "decimate_2": _summary(dec)}), flush=True)


def pyramid_end_to_end(rounds):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(2520, 1920, 3), dtype=np.uint8)
    levels = len(pconv.ops.pyramid_sizes(1920, 2520))
    pyr = pconv.Pyramid(1920, 2520, "rgb", levels)

    def by_hand():
        outs = [img]
        for _ in range(levels - 1):
            outs.append(np.ascontiguousarray(pconv.convolve(outs[-1], 2, backend="hip")[::2, ::2]))
        return outs

    # the same with one persistent Engine per level (convolve's cache holds 8 engines, fewer than the
    # levels of this image, so by_hand rebuilds engines on every call): full downloads + host slicing alone
    engines = [pconv.Engine(w, h, "rgb") for w, h in pconv.ops.pyramid_sizes(1920, 2520)[:-1]]

    def by_hand_engines():
        outs = [img]
        for e in engines:
            outs.append(np.ascontiguousarray(e.run_numpy(outs[-1], 2)[::2, ::2]))
        return outs

    for _ in range(3):
        a, b, c = by_hand(), pyr(img), by_hand_engines()
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c))
    hand, dev, own = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        by_hand()
        t1 = time.perf_counter()
        pyr(img)
        t2 = time.perf_counter()
        by_hand_engines()
        t3 = time.perf_counter()
        hand.append((t1 - t0) * 1e3)
        dev.append((t2 - t1) * 1e3)
        own.append((t3 - t2) * 1e3)
    print(json.dumps({"what": "pyramid 1920x2520 rgb, reps 2", "levels": levels,
                      "convolve_and_host_slicing": _summary(hand),
                      "persistent_engines_and_host_slicing": _summary(own), "Pyramid": _summary(dev)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--copies", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--skip-big", action="store_true", help="leave the 32768^2 grey frame (1 GiB) out")
    ap.add_argument("--only-pyramid", action="store_true", help="the pyramid comparison alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decimate_cost.py measures on a GPU; none is visible")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if a.only_pyramid:
        return pyramid_end_to_end(a.rounds)
    kernel_alone("1920x2520 rgb", 1920, 2520, 3, 2, 1, a.launches, a.copies)
    kernel_alone("1920x2520 rgb", 1920, 2520, 3, 4, 1, a.launches, a.copies)
    kernel_alone("64 x 320x240 rgb", 320, 240, 3, 2, 64, a.launches, a.copies)
    if not a.skip_big:
        kernel_alone("32768^2 grey", 32768, 32768, 1, 2, 1, max(10, a.launches // 10), 5)
    engine_end_to_end(a.rounds)
    pyramid_end_to_end(a.rounds)


if __name__ == "__main__":
    main()
