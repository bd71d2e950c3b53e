"""Compaction on a real MI355X: ``BatchEngine.run_until_stable(compact=True)``
retires converged images from the fused and the residual launches, and returns
exactly what ``compact=False`` returns — every image ends as the single-image
NumPy-backend run of that image ends, in bytes and in ``StableInfo``.

``stats.image_launches`` is the observable that work was retired; it is held to
the formula of batch_compact_formula.py (checked on hand-made cases in
test_batch_compact_cpu.py).  fuse = 8 makes one launch per chunk of 8 (the
newest frame flips every chunk), fuse = 4 two (it never flips): a stale frame
of a retired image would show under one of them.

Exact integers and exact bytes only.  Tuning is off, shapes are forced."""
import numpy as np
import pytest

import batch_modes_recipe as modes
from batch_compact_formula import converged_at, expected_image_launches
from batch_converge_recipe import BORDERS, GEOMS, NAME, RUNS, check_spread, oracle, recipe

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def forced(native):
    prev = native.set_autotune(False)
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    yield
    native.set_swar_shape(0, 0, 0)
    native.set_float_shape(0, 0)
    native.set_autotune(prev)


@pytest.mark.parametrize("fuse", [8, 4])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_run_until_stable_compact(pconv_mod, c, h, w, filt, border, fuse):
    check_spread(pconv_mod, c, h, w, filt, border)  # on the oracle alone: images stop at different checks
    stack = recipe(c, h, w)
    n = len(stack)
    eng = pconv_mod.BatchEngine(w, h, NAME[c], n, filt, fuse=fuse, border=border)
    assert eng.fuse == fuse
    for max_reps, k in RUNS:
        refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, max_reps, k)
        case = (filt, border, fuse, max_reps, k)
        off, off_infos = eng.run_until_stable(stack, max_reps, check_every=k, compact=False)
        off_stats = (eng.stats.image_launches, eng.stats.launches)
        on, on_infos = eng.run_until_stable(stack, max_reps, check_every=k, compact=True)
        on_stats = (eng.stats.image_launches, eng.stats.launches)
        assert isinstance(on, np.ndarray) and on_infos == rinfos and off_infos == rinfos, case
        for b in range(n):
            assert np.array_equal(on[b], refs[b]), case + (b,)
        assert np.array_equal(on, off), case
        # the resident frames are the returned images, retired ones included
        assert eng.residual().tolist() == [i.residual for i in rinfos], case
        conv = converged_at(rinfos)
        assert off_stats == expected_image_launches(max_reps, k, fuse, conv, False), case
        assert on_stats == expected_image_launches(max_reps, k, fuse, conv, True), case
        assert off_stats[0] == off_stats[1] * n and on_stats[1] == off_stats[1], case
        if (max_reps, k) == (400, 8):
            assert on_stats[0] < on_stats[1] * n, case


@pytest.mark.parametrize("fuse", [8, 4])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_a_plain_run_after_a_compacted_one(pconv_mod, native, c, h, w, filt, border, fuse):
    """Both frames of a retired image hold its bytes, and the open images go
    on: 3 more repetitions of the whole batch after a compacted (24, 8) run."""
    stack = np.ascontiguousarray(recipe(c, h, w)).copy()
    n = len(stack)
    refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, 24, 8)
    assert any(i.converged and i.checks < 3 for i in rinfos)  # some image IS retired before the loop ends
    eng = native.BatchEngine(w, h, NAME[c], n, filt, fuse=fuse, border=border)
    eng.upload(stack.reshape(-1), n)
    st = eng.run_until_stable(24, 8, n, compact=True)
    assert [(s[0], s[1], s[2], s[3]) for s in st] == [(i.reps_done, i.converged, i.residual, i.checks) for i in rinfos]
    got = np.empty_like(stack)
    eng.download(got.reshape(-1), n)
    eng.synchronize()
    assert np.array_equal(got, np.stack(refs))
    eng.run(3, n)
    assert eng.stats.image_launches == eng.stats.launches * n  # the table does not outlive the call
    eng.download(got.reshape(-1), n)
    eng.synchronize()
    for b in range(n):
        assert np.array_equal(got[b], pconv_mod.numpy_convolve(refs[b], 3, filt, border=border)), (filt, border, fuse, b)
    # ... and a compacted run of a part of the batch afterwards
    eng.upload(stack[2:6].reshape(-1), 4)
    st = eng.run_until_stable(24, 8, 4, compact=True)
    assert [s[0] for s in st] == [i.reps_done for i in rinfos[2:6]]
    eng.download(got[:4].reshape(-1), 4)
    eng.synchronize()
    assert np.array_equal(got[:4], np.stack(refs[2:6]))


@pytest.mark.parametrize("fuse", [8, 4])
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_nothing_converges_and_everything_converges_at_once(pconv_mod, c, h, w, filt, fuse):
    """Neither loop ever builds a table: nothing is found fixed, or the loop
    ends at the check that finds everything fixed."""
    border = "replicate"
    stack = recipe(c, h, w)
    eng = pconv_mod.BatchEngine(w, h, NAME[c], 4, filt, fuse=fuse, border=border)
    # the three uniform random images, 20 repetitions (8 + 8 + 4): none is at its fixed point
    part = np.ascontiguousarray(stack[2:5])
    res = [pconv_mod.convolve_until_stable(im, 20, filt, check_every=8, backend="numpy", border=border) for im in part]
    assert not any(r[1].converged for r in res)
    out, infos = eng.run_until_stable(part, 20, check_every=8, compact=True)
    assert infos == [r[1] for r in res] and np.array_equal(out, np.stack([r[0] for r in res]))
    want = expected_image_launches(20, 8, fuse, [None] * 3, True)
    assert (eng.stats.image_launches, eng.stats.launches) == want and want[0] == want[1] * 3
    # all 255, all 0, all 255: under the replicate border at a fixed point by the first check (box/9 in
    # float32 takes 255 to 254 first)
    flat = np.ascontiguousarray(stack[[0, 1, 0]])
    res = [pconv_mod.convolve_until_stable(im, 400, filt, check_every=8, backend="numpy", border=border) for im in flat]
    out, infos = eng.run_until_stable(flat, 400, check_every=8, compact=True)
    assert infos == [r[1] for r in res] and np.array_equal(out, np.stack([r[0] for r in res]))
    assert [(i.reps_done, i.converged, i.checks) for i in infos] == [(8, True, 1)] * 3
    want = expected_image_launches(400, 8, fuse, [1, 1, 1], True)
    assert (eng.stats.image_launches, eng.stats.launches) == want and want[0] == want[1] * 3


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{NAME[g[0]]}-{g[3]}")
def test_run_images_until_stable_compact(pconv_mod, geom):
    c, h, w, filt = geom
    border = "replicate"
    stack = recipe(c, h, w)
    # the recipe's images cropped to differing sizes (image k loses k % 3 rows and k % 4 columns)
    imgs = [np.ascontiguousarray(stack[k][:h - k % 3, :w - k % 4]) for k in range(len(stack))]
    eng = pconv_mod.BatchEngine(w, h, NAME[c], len(imgs), filt, fuse=8, border=border)
    for max_reps, k in RUNS:
        single = [pconv_mod.convolve_until_stable(im, max_reps, filt, check_every=k, backend="numpy", border=border)
                  for im in imgs]
        outs, infos = eng.run_images_until_stable(imgs, max_reps, k, compact=True)
        stats = (eng.stats.image_launches, eng.stats.launches)
        held = eng.residual_images()
        for b, (ro, ri) in enumerate(single):
            assert np.array_equal(outs[b], ro) and infos[b] == ri, (geom, max_reps, b, infos[b], ri)
            assert int(held[b]) == ri.residual
        assert stats == expected_image_launches(max_reps, k, 8, converged_at(infos), True), (geom, max_reps)
        offs, off_infos = eng.run_images_until_stable(imgs, max_reps, k)
        assert off_infos == infos and all(np.array_equal(a, b) for a, b in zip(outs, offs))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c", modes.CHANNELS)
def test_one_engine_through_mixed_plain_and_mixed_again(pconv_mod, c, border):
    """The modes share the engine's staged tables and its per-image copies: one
    engine runs mixed sizes, a plain stack and other mixed sizes in a row, every
    run compacting, and each image ends as its single-image CPU run ends."""
    eng = pconv_mod.BatchEngine(modes.W, modes.H, NAME[c], modes.CAPACITY, modes.FILTER, fuse=modes.FUSE, border=border)
    assert eng.fuse == modes.FUSE
    for step, ((kind, imgs), (refs, rinfos)) in enumerate(zip(modes.steps(c, border), modes.oracle(pconv_mod, c, border))):
        case = (c, border, step)
        if kind == "stack":
            outs, infos = eng.run_until_stable(np.stack(imgs), modes.MAX_REPS, modes.CHECK_EVERY, compact=True)
            held = eng.residual()
        else:
            outs, infos = eng.run_images_until_stable(imgs, modes.MAX_REPS, modes.CHECK_EVERY, compact=True)
            held = eng.residual_images()
        stats = (eng.stats.image_launches, eng.stats.launches)
        assert infos == rinfos, case
        assert len(outs) == len(refs) and all(np.array_equal(o, r) for o, r in zip(outs, refs)), case
        assert held.tolist() == [i.residual for i in rinfos], case
        assert stats == expected_image_launches(modes.MAX_REPS, modes.CHECK_EVERY, modes.FUSE, converged_at(infos),
                                                True), case
        if modes.retires(infos):
            assert stats[0] < stats[1] * len(imgs), case


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_public_entries_on_the_hip_backend(pconv_mod, c, h, w, filt, border):
    import torch

    stack = recipe(c, h, w)
    kw = dict(filter=filt, check_every=8, backend="hip", fuse=4, border=border)
    for max_reps in (400, 24):
        refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, max_reps, 8)
        off, off_infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, **kw)
        for bs in (None, 3):  # one engine of 7; chunks of 3, 3 and 1, each with its own loop and table
            on, on_infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, compact=True, batch_size=bs, **kw)
            assert on_infos == off_infos == rinfos and np.array_equal(on, off), (filt, border, max_reps, bs)
            assert np.array_equal(on, np.stack(refs))
    dev = torch.from_numpy(stack.copy()).cuda()
    on, on_infos = pconv_mod.convolve_batch_until_stable(dev, 24, compact=True, **kw)
    assert on.is_cuda and on_infos == rinfos and np.array_equal(on.cpu().numpy(), np.stack(refs))
    imgs = [np.ascontiguousarray(stack[k][:h - k % 3, :w - k % 4]) for k in range(len(stack))]
    off, off_infos = pconv_mod.convolve_many_until_stable(imgs, 400, **kw)
    on, on_infos = pconv_mod.convolve_many_until_stable(imgs, 400, compact=True, **kw)
    assert on_infos == off_infos and len(on) == len(imgs)
    for im, a, b, info in zip(imgs, on, off, on_infos):
        assert np.array_equal(a, b)
        ro, ri = pconv_mod.convolve_until_stable(im, 400, filt, check_every=8, backend="numpy", border=border)
        assert np.array_equal(a, ro) and info == ri
