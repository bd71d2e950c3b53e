"""``compact=`` without a GPU: the ``numpy`` and ``cpu`` backends accept the
argument and ignore it (they loop per image and already stop each image at its
own fixed point), so both settings return identical stacks and ``StableInfo``
lists; and the ``image_launches`` formula the GPU test holds the engine to
(batch_compact_formula.py) on hand-made cases.

Exact integers and exact bytes only."""
import numpy as np
import pytest

import batch_modes_recipe as modes
from batch_compact_formula import chunk_launches, converged_at, expected_image_launches
from batch_converge_recipe import BORDERS, GEOMS, check_spread, oracle, recipe

BACKENDS = ["numpy", "cpu"]
RUNS = [(400, 8), (24, 8)]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_batch_until_stable_ignores_compact(pconv_mod, c, h, w, filt, backend, border):
    stack = recipe(c, h, w)
    for max_reps, k in RUNS:
        refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, max_reps, k)
        kw = dict(filter=filt, check_every=k, backend=backend, border=border)
        off, off_infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, compact=False, **kw)
        on, on_infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, compact=True, **kw)
        case = (backend, border, filt, max_reps, k)
        assert isinstance(on, np.ndarray) and on.dtype == np.uint8 and on.shape == stack.shape, case
        assert np.array_equal(on, off) and on_infos == off_infos, case
        assert np.array_equal(on, np.stack(refs)) and on_infos == rinfos, case
        # the default is off, and is the call without the argument
        dflt, dflt_infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, **kw)
        assert np.array_equal(dflt, off) and dflt_infos == off_infos, case


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_many_until_stable_ignores_compact(pconv_mod, c, h, w, filt, backend, border):
    stack = recipe(c, h, w)
    # the recipe's images cropped to differing sizes (image k loses k % 3 rows and k % 4 columns)
    imgs = [np.ascontiguousarray(stack[k][:h - k % 3, :w - k % 4]) for k in range(len(stack))]
    assert len({im.shape for im in imgs}) >= 5
    kw = dict(filter=filt, check_every=8, backend=backend, border=border)
    off, off_infos = pconv_mod.convolve_many_until_stable(imgs, 24, compact=False, **kw)
    on, on_infos = pconv_mod.convolve_many_until_stable(imgs, 24, compact=True, **kw)
    assert on_infos == off_infos and len(on) == len(imgs)
    for im, a, b, info in zip(imgs, on, off, on_infos):
        assert a.shape == im.shape and np.array_equal(a, b)
        ro, ri = pconv_mod.convolve_until_stable(im, 24, filt, check_every=8, backend="numpy", border=border)
        assert np.array_equal(a, ro) and info == ri


def test_formula_on_hand_made_cases():
    # three chunks of 8 at fuse 4 (2 launches each): fixed at check 1 -> chunks 1-2, at check 2 -> chunks 1-3
    assert chunk_launches(24, 8, 4, [1, 2, None]) == [2, 2, 2]
    assert expected_image_launches(24, 8, 4, [1, 2, None], True) == (4 + 6 + 6, 6)
    assert expected_image_launches(24, 8, 4, [1, 2, None], False) == (18, 6)
    # all fixed at the first check: the chunk in flight is the last, nothing was retired
    assert chunk_launches(400, 8, 8, [1, 1]) == [1, 1]
    assert expected_image_launches(400, 8, 8, [1, 1], True) == (4, 2)
    assert expected_image_launches(400, 8, 8, [1, 1], False) == (4, 2)
    # a shorter last chunk counts with its own launches: 8 + 2 repetitions at fuse 4 are 2 + 1
    assert chunk_launches(10, 8, 4, [1, None]) == [2, 1]
    assert expected_image_launches(10, 8, 4, [1, None], True) == (6, 3)
    # 8 + 8 + 4 at fuse 4 are 2 + 2 + 1: the image fixed at check 1 misses the last chunk only
    assert chunk_launches(20, 8, 4, [1, None]) == [2, 2, 1]
    assert expected_image_launches(20, 8, 4, [1, None], True) == (4 + 5, 5)
    # nothing converges: compaction changes nothing
    assert expected_image_launches(20, 8, 4, [None] * 3, True) == expected_image_launches(20, 8, 4, [None] * 3, False)
    # the loop ends at the check that finds the last image fixed, with one chunk in flight
    assert chunk_launches(400, 8, 8, [1, 3, 5]) == [1] * 6
    assert expected_image_launches(400, 8, 8, [1, 3, 5], True) == (2 + 4 + 6, 6)
    # an image fixed at the very last check of a max_reps-bounded loop is never retired
    assert chunk_launches(16, 8, 8, [2, None]) == [1, 1]
    assert expected_image_launches(16, 8, 8, [2, None], True) == (4, 2)
    # no repetitions at all
    assert expected_image_launches(0, 8, 8, [None, None], True) == (0, 0)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_formula_on_the_recipe(pconv_mod, c, h, w, filt, border):
    """On the oracle's own results: the (400, 8) run of the 7 images would
    retire work (strictly fewer image launches than launches x 7)."""
    check_spread(pconv_mod, c, h, w, filt, border)
    _, infos = oracle(pconv_mod, c, h, w, filt, border, 400, 8)
    for fuse in (8, 4):
        on, launches = expected_image_launches(400, 8, fuse, converged_at(infos), True)
        off, _ = expected_image_launches(400, 8, fuse, converged_at(infos), False)
        assert off == launches * len(infos) and 0 < on < off


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c", modes.CHANNELS)
def test_modes_recipe(pconv_mod, c, border):
    """The three steps test_gpu_batch_compact.py takes one engine through, on
    the oracle alone: the sizes fit the engine, the CPU backends agree on every
    image, and every step has something to retire and something still open."""
    plan = modes.steps(c, border)
    assert [kind for kind, _ in plan] == ["images", "stack", "images"]
    assert [(im.shape[1], im.shape[0]) for im in plan[0][1]] == [(67, 33), (5, 31), (64, 32), (1, 1)]
    assert [(im.shape[1], im.shape[0]) for im in plan[1][1]] == [(modes.W, modes.H)] * 3
    assert len({im.shape for im in plan[2][1]}) == 3 and {im.shape for im in plan[2][1]}.isdisjoint(
        {im.shape for im in plan[0][1]})
    flat = plan[1][1][1]
    assert int(flat.min()) == int(flat.max())  # the stack's constant image
    for (kind, imgs), (outs, infos) in zip(plan, modes.oracle(pconv_mod, c, border)):
        assert 1 <= len(imgs) <= modes.CAPACITY
        for im, out, info in zip(imgs, outs, infos):
            assert im.dtype == np.uint8 and im.ndim == (2 if c == 1 else 3) and im.shape[:2] <= (modes.H, modes.W)
            ro, ri = pconv_mod.convolve_until_stable(im, modes.MAX_REPS, modes.FILTER, check_every=modes.CHECK_EVERY,
                                                     backend="numpy", border=border)
            assert np.array_equal(out, ro) and info == ri
        assert modes.retires(infos) and not all(i.converged for i in infos), (kind, infos)
        on = expected_image_launches(modes.MAX_REPS, modes.CHECK_EVERY, modes.FUSE, converged_at(infos), True)
        assert 0 < on[0] < on[1] * len(imgs)
    if border == "replicate":
        assert modes.oracle(pconv_mod, c, border)[1][1][1] == pconv_mod.StableInfo(modes.CHECK_EVERY, True, 0, 1)
