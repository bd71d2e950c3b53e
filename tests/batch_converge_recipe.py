"""The 7-image batch both batch-convergence test files run to the fixed point,
and its per-image oracle (the NumPy backend's ``convolve_until_stable``).

Per geometry, fixed seed: all 255, all 0, three uniform random in [0, 256),
one uniform random in [0, 4), one whose left half of columns is 255 and right
half 0.  The images reach their fixed points after very different numbers of
repetitions, which ``check_spread`` asserts on the oracle's own results: a
batch whose images all stop at the same check could not tell a per-image
decision from a whole-batch one."""
import numpy as np

GEOMS = [(1, 9, 13, "gaussian"), (3, 21, 13, "box")]  # (channels, height, width, filter)
BORDERS = ["zero", "replicate"]
RUNS = [(400, 8), (24, 8), (10, 8)]  # (max_reps, check_every)
NAME = {1: "grey", 3: "rgb", 4: "rgba"}

_STACK = {}
_ORACLE = {}


def recipe(c, h, w):
    key = (c, h, w)
    if key not in _STACK:
        rng = np.random.default_rng(20240 + 7919 * c + 104729 * h + w)
        shape = (h, w, c) if c > 1 else (h, w)
        imgs = [np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)]
        imgs += [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(3)]
        imgs.append(rng.integers(0, 4, size=shape, dtype=np.uint8))
        half = np.zeros(shape, np.uint8)
        half[:, :w // 2] = 255
        imgs.append(half)
        _STACK[key] = np.stack(imgs)
        _STACK[key].setflags(write=False)
    return _STACK[key]


def oracle(pconv_mod, c, h, w, filt, border, max_reps, k):
    """([out_b], [StableInfo_b]) of the per-image NumPy-backend runs, computed once."""
    key = (c, h, w, filt, border, max_reps, k)
    if key not in _ORACLE:
        res = [pconv_mod.convolve_until_stable(img, max_reps, filt, check_every=k, backend="numpy", border=border)
               for img in recipe(c, h, w)]
        _ORACLE[key] = ([r[0] for r in res], [r[1] for r in res])
    return _ORACLE[key]


def check_spread(pconv_mod, c, h, w, filt, border):
    """The batch is not degenerate: the (400, 8) run stops at >= 3 distinct
    repetition counts, the (24, 8) run has converged and unconverged images."""
    _, long_ = oracle(pconv_mod, c, h, w, filt, border, 400, 8)
    assert len({i.reps_done for i in long_}) >= 3, [i.reps_done for i in long_]
    _, short = oracle(pconv_mod, c, h, w, filt, border, 24, 8)
    conv = [i.converged for i in short]
    assert any(conv) and not all(conv), conv
