#!/usr/bin/env python3
"""Cost of the unsharp mask (docs/PERFORMANCE.md 3.9), on the GPU.

1. k_unsharp alone between stream events (native.launch_unsharp(timed=...),
   out of place) on engine-like pitched frames of the 1920x2520 rgb image at
   depth 8 and depth 16, beside the row-copy kernel (native.time_copy_rows)
   device to device on the same frame in the same session.  The copy moves two
   thirds of the kernel's bytes (one read and one write per byte against two
   reads and one write): the yardstick is 1.5 x the copy.
2. Engine.unsharp(img, 40, 1.0) end to end from NumPy, beside
   Engine.run_numpy(img, 40) on the same engine, and beside run_numpy plus the
   three-pass NumPy combine on the host (int32 temporaries and a clip),
   alternating, host clock around whole calls.

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


def kernel_alone(w, h, channels, depth, launches):
    n = pconv.native
    rb = w * channels * (depth // 8)
    pitch = _ceil(16 + _ceil(rb, 16) * 16 + 32, 128) * 128
    size = (h + 2) * pitch
    orig = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
    blur = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
    dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    off = pitch + 16
    stream = torch.cuda.current_stream().cuda_stream
    args = (orig.data_ptr() + off, pitch, blur.data_ptr() + off, pitch, dst.data_ptr() + off, pitch, rb, h)
    kw = dict(depth=depth, k=16, threshold=0, stream=stream)
    torch.cuda.synchronize()
    n.launch_unsharp(*args, **kw, timed=5)  # warm-up: code object, caches
    copy_args = (orig.data_ptr() + off, pitch, dst.data_ptr() + off, pitch, rb, h)
    n.time_copy_rows(*copy_args, timed=5)
    # alternate the two in blocks, so that a drift of the machine meets both
    ms_k, ms_c = [], []
    for _ in range(4):
        ms_k += n.launch_unsharp(*args, **kw, timed=launches // 4)
        ms_c += n.time_copy_rows(*copy_args, timed=launches // 4)
    k, c = _summary(ms_k), _summary(ms_c)
    moved = 3 * rb * h
    print(json.dumps({"what": "k_unsharp", "case": f"{w}x{h} x{channels} depth {depth}", "frame_bytes": rb * h,
                      "kernel": k, "copy_rows_d2d": c, "ratio_of_medians": round(k["median_ms"] / c["median_ms"], 3),
                      "kernel_GBps": round(moved / k["median_ms"] / 1e6, 1),
                      "copy_GBps": round(2 * rb * h / c["median_ms"] / 1e6, 1)}), flush=True)


def host_combine(x, b, k=16):
    """What a user of the blur alone writes: three passes, int32 temporaries, a clip."""
    xs = x.astype(np.int32)
    num = xs * (16 + k) - b.astype(np.int32) * k + 8
    return np.clip(num >> 4, 0, 255).astype(np.uint8)


def engine_end_to_end(rounds):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(2520, 1920, 3), dtype=np.uint8)
    eng = pconv.Engine(1920, 2520, "rgb")
    for _ in range(3):
        a = host_combine(img, eng.run_numpy(img, 40))
        b = eng.unsharp(img, 40, 1.0)
    assert np.array_equal(a, b)
    plain, host, dev = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = eng.run_numpy(img, 40)
        t1 = time.perf_counter()
        host_combine(img, out)
        t2 = time.perf_counter()
        eng.unsharp(img, 40, 1.0)
        t3 = time.perf_counter()
        plain.append((t1 - t0) * 1e3)
        host.append((t2 - t0) * 1e3)
        dev.append((t3 - t2) * 1e3)
    print(json.dumps({"what": "Engine 1920x2520 rgb x40 from NumPy", "run_numpy": _summary(plain),
                      "run_numpy_plus_host_combine": _summary(host), "Engine.unsharp": _summary(dev)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unsharp_cost.py measures on a GPU; none is visible")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    kernel_alone(1920, 2520, 3, 8, a.launches)
    kernel_alone(1920, 2520, 3, 16, a.launches)
    engine_end_to_end(a.rounds)


if __name__ == "__main__":
    main()
