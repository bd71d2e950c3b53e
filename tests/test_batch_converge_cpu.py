"""Batches to their fixed points without a GPU: ``convolve_batch_until_stable``
and ``residual_batch`` on the ``numpy`` / ``cpu`` / ``omp`` backends.

The contract is per image: entry b of a batch result is what the single-image
call returns for image b, in bytes and in ``StableInfo``.  The oracle is the
NumPy backend's single-image ``convolve_until_stable`` (batch_converge_recipe).

Exact integers and exact bytes only."""
import numpy as np
import pytest
import torch

from batch_converge_recipe import BORDERS, GEOMS, RUNS, check_spread, oracle, recipe

BACKENDS = ["numpy", "cpu", "omp"]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_recipe_is_not_degenerate(pconv_mod, c, h, w, filt, border):
    check_spread(pconv_mod, c, h, w, filt, border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_batch_until_stable_equals_single_images(pconv_mod, c, h, w, filt, backend, border):
    stack = recipe(c, h, w)
    for max_reps, k in RUNS + [(0, 8)]:
        refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, max_reps, k)
        case = (backend, border, filt, max_reps, k)
        out, infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, filt, check_every=k, backend=backend,
                                                           border=border)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == stack.shape, case
        assert infos == rinfos, case
        for b in range(len(stack)):
            assert np.array_equal(out[b], refs[b]), case + (b,)
            # ... which is the single-image call of the same backend
            one, info = pconv_mod.convolve_until_stable(stack[b], max_reps, filt, check_every=k, backend=backend,
                                                        border=border)
            assert info == infos[b] and np.array_equal(one, out[b]), case + (b,)


@pytest.mark.parametrize("backend", BACKENDS)
def test_containers(pconv_mod, backend):
    c, h, w, filt = GEOMS[1]
    stack = recipe(c, h, w)
    refs, rinfos = oracle(pconv_mod, c, h, w, filt, "replicate", 24, 8)
    kw = dict(filter=filt, check_every=8, backend=backend, border="replicate")
    # a sequence of images is stacked; batch_size is a GPU matter and changes nothing here
    out, infos = pconv_mod.convolve_batch_until_stable([stack[b] for b in range(len(stack))], 24, batch_size=3, **kw)
    assert isinstance(out, np.ndarray) and np.array_equal(out, np.stack(refs)) and infos == rinfos
    # a CPU tensor comes back as a CPU tensor
    out, infos = pconv_mod.convolve_batch_until_stable(torch.from_numpy(stack.copy()), 24, **kw)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and not out.is_cuda
    assert np.array_equal(out.numpy(), np.stack(refs)) and infos == rinfos
    # an empty batch has a geometry and no images
    for empty in (np.zeros((0, h, w, c), np.uint8), np.zeros((0, h, w), np.uint8)):
        out, infos = pconv_mod.convolve_batch_until_stable(empty, 24, **kw)
        assert isinstance(out, np.ndarray) and out.shape == empty.shape and out.dtype == np.uint8 and infos == []
        res = pconv_mod.residual_batch(empty, filt, backend=backend, border="replicate")
        assert res.shape == (0,) and res.dtype == np.int64
    out, infos = pconv_mod.convolve_batch_until_stable(torch.zeros((0, h, w), dtype=torch.uint8), 24, **kw)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (0, h, w) and infos == []


def test_default_check_every_is_the_single_image_default(pconv_mod):
    c, h, w, filt = GEOMS[0]
    stack = recipe(c, h, w)
    out, infos = pconv_mod.convolve_batch_until_stable(stack, 400, filt, backend="numpy", border="replicate")
    for b in range(len(stack)):
        one, info = pconv_mod.convolve_until_stable(stack[b], 400, filt, backend="numpy", border="replicate")
        assert info == infos[b] and info.reps_done % 32 == 0 and np.array_equal(one, out[b])


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_residual_batch_equals_single_images(pconv_mod, c, h, w, filt, backend, border):
    stack = recipe(c, h, w)
    want = [pconv_mod.numpy_residual(stack[b], filt, border) for b in range(len(stack))]
    assert want[1] == 0 and sum(1 for x in want if x) >= 4
    got = pconv_mod.residual_batch(stack, filt, backend=backend, border=border)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (len(stack),)
    assert got.tolist() == want
    assert got.tolist() == [pconv_mod.residual(stack[b], filt, backend=backend, border=border)
                            for b in range(len(stack))]
    got = pconv_mod.residual_batch([torch.from_numpy(stack[b].copy()) for b in range(3)], filt, backend=backend,
                                   border=border)
    assert got.dtype == np.int64 and got.tolist() == want[:3]


def test_rejections(pconv_mod):
    z = np.zeros((2, 7, 9), np.uint8)
    with pytest.raises(ValueError, match="max_reps"):
        pconv_mod.convolve_batch_until_stable(z, -1, backend="numpy")
    for k in (0, -3):
        with pytest.raises(ValueError, match="check_every"):
            pconv_mod.convolve_batch_until_stable(z, 5, check_every=k, backend="numpy")
    with pytest.raises(ValueError, match="batch_size"):
        pconv_mod.convolve_batch_until_stable(z, 5, backend="numpy", batch_size=0)
    with pytest.raises(ValueError, match="backend"):
        pconv_mod.convolve_batch_until_stable(z, 5, backend="cuda")
    with pytest.raises(ValueError, match="backend"):
        pconv_mod.residual_batch(z, backend="cuda")
    with pytest.raises(ValueError):
        pconv_mod.convolve_batch_until_stable(z, 5, backend="numpy", border="mirror")
    with pytest.raises(ValueError, match="batch shape"):
        pconv_mod.convolve_batch_until_stable(z[0], 5, backend="numpy")
    with pytest.raises(ValueError, match="one shape"):
        pconv_mod.residual_batch([z[0], np.zeros((7, 10), np.uint8)], backend="numpy")
    with pytest.raises(ValueError):
        pconv_mod.convolve_batch_until_stable([], 5, backend="numpy")
    for bad in (np.zeros((2, 7, 9), np.int16), torch.zeros((2, 7, 9), dtype=torch.float32)):
        with pytest.raises(TypeError, match="uint8"):
            pconv_mod.convolve_batch_until_stable(bad, 5, backend="numpy")
        with pytest.raises(TypeError, match="uint8"):
            pconv_mod.residual_batch(bad, backend="numpy")
