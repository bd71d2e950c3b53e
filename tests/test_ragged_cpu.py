"""Images of different sizes without a GPU: ``convolve_many``,
``convolve_many_until_stable`` and ``residual_many`` on the ``numpy``, ``cpu``
and ``omp`` backends equal the per-image calls, and ``size_buckets`` keeps its
contract on a seeded set of sizes and on the adversarial ones."""
import numpy as np
import pytest
import torch

BACKENDS = ["numpy", "cpu", "omp"]
BORDERS = ["zero", "replicate"]
SIZES = [(1, 1), (7, 5), (1, 9), (12, 1), (16, 16), (33, 20), (2, 3)]  # (width, height), from 1x1 up


def _images(c, seed=5):
    rng = np.random.default_rng(seed + c)
    out = []
    for w, h in SIZES:
        shape = (h, w, c) if c > 1 else (h, w)
        out.append(rng.integers(0, 256, size=shape, dtype=np.uint8))
    return out


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("backend", BACKENDS)
def test_convolve_many_equals_per_image(pconv_mod, backend, c, filt, border):
    imgs = _images(c)
    got = pconv_mod.convolve_many(imgs, 5, filt, backend=backend, border=border)
    assert isinstance(got, list) and len(got) == len(imgs)
    for im, g in zip(imgs, got):  # input order
        ref = pconv_mod.convolve(im, 5, filt, backend=backend, border=border)
        assert isinstance(g, np.ndarray) and g.shape == im.shape and g.dtype == np.uint8
        assert np.array_equal(g, ref)
        assert np.array_equal(g, pconv_mod.numpy_convolve(im, 5, filt, border=border))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_until_stable_and_residual_many(pconv_mod, backend, border):
    for c, filt in ((1, "gaussian"), (3, "box")):
        imgs = _images(c)
        imgs[0] = np.zeros_like(imgs[0])  # a fixed point from the start
        outs, infos = pconv_mod.convolve_many_until_stable(imgs, 40, filt, check_every=8, backend=backend,
                                                           border=border)
        assert len(outs) == len(infos) == len(imgs)
        res = pconv_mod.residual_many(imgs, filt, backend=backend, border=border)
        assert res.dtype == np.int64 and res.shape == (len(imgs),)
        for i, im in enumerate(imgs):
            ro, ri = pconv_mod.convolve_until_stable(im, 40, filt, check_every=8, backend=backend, border=border)
            assert np.array_equal(outs[i], ro) and infos[i] == ri, (backend, border, c, i)
            assert int(res[i]) == pconv_mod.residual(im, filt, backend=backend, border=border)
        assert infos[0].converged and infos[0].checks == 1


def test_containers_order_and_empty(pconv_mod):
    imgs = _images(3)
    tens = [torch.from_numpy(im) for im in imgs]
    got = pconv_mod.convolve_many(tens, 3, backend="numpy", border="replicate")
    assert all(isinstance(g, torch.Tensor) and g.dtype == torch.uint8 and g.device == tens[0].device for g in got)
    for im, g in zip(imgs, got):
        assert np.array_equal(g.numpy(), pconv_mod.numpy_convolve(im, 3, "gaussian", border="replicate"))
    # a generator, and reversed order in gives reversed order out
    rev = pconv_mod.convolve_many((im for im in reversed(imgs)), 3, backend="cpu")
    assert [r.shape for r in rev] == [im.shape for im in reversed(imgs)]
    # (H, W) and (H, W, 1) are both grey and keep their shapes
    g2, g3 = np.full((4, 6), 200, np.uint8), np.full((3, 2, 1), 100, np.uint8)
    out = pconv_mod.convolve_many([g2, g3], 2, backend="numpy")
    assert out[0].shape == (4, 6) and out[1].shape == (3, 2, 1)
    assert np.array_equal(out[1], pconv_mod.numpy_convolve(g3, 2, "gaussian"))
    for backend in BACKENDS + ["auto"]:
        assert pconv_mod.convolve_many([], 4, backend=backend) == []
        assert pconv_mod.convolve_many_until_stable([], 4, backend=backend) == ([], [])
        r = pconv_mod.residual_many([], backend=backend)
        assert r.shape == (0,) and r.dtype == np.int64
    assert pconv_mod.convolve_many(imgs, 0, backend="numpy")[1].tobytes() == imgs[1].tobytes()


def test_rejections(pconv_mod):
    imgs = _images(3)
    with pytest.raises(ValueError, match="one channel count"):
        pconv_mod.convolve_many([imgs[0], _images(1)[0]], 1, backend="numpy")
    with pytest.raises(TypeError, match="all NumPy arrays or all torch tensors"):
        pconv_mod.convolve_many([imgs[0], torch.from_numpy(imgs[1])], 1, backend="numpy")
    with pytest.raises(TypeError, match="uint8"):
        pconv_mod.convolve_many([imgs[0].astype(np.float32)], 1, backend="numpy")
    with pytest.raises(TypeError, match="uint8"):
        pconv_mod.convolve_many([torch.zeros(3, 3, dtype=torch.float32)], 1, backend="numpy")
    with pytest.raises(TypeError, match="sequence of images"):
        pconv_mod.convolve_many(np.zeros((2, 3, 3), np.uint8), 1, backend="numpy")
    with pytest.raises(ValueError, match="unsupported image shape"):
        pconv_mod.convolve_many([np.zeros((2, 3, 2), np.uint8)], 1, backend="numpy")
    with pytest.raises(ValueError, match="reps"):
        pconv_mod.convolve_many(imgs, -1, backend="numpy")
    with pytest.raises(ValueError, match="unknown backend"):
        pconv_mod.convolve_many(imgs, 1, backend="cuda")
    with pytest.raises(ValueError, match="batch_size"):
        pconv_mod.convolve_many(imgs, 1, backend="numpy", batch_size=0)
    with pytest.raises(ValueError, match="min_fill"):
        pconv_mod.convolve_many(imgs, 1, backend="numpy", min_fill=1.5)
    with pytest.raises(ValueError, match="border"):
        pconv_mod.residual_many(imgs, backend="numpy", border="mirror")
    with pytest.raises(ValueError, match="max_reps"):
        pconv_mod.convolve_many_until_stable(imgs, -1, backend="numpy")
    with pytest.raises(ValueError, match="check_every"):
        pconv_mod.convolve_many_until_stable(imgs, 4, check_every=0, backend="numpy")
    # the same-size entry point keeps its contract
    with pytest.raises(ValueError, match="one shape"):
        pconv_mod.convolve_batch([imgs[0], imgs[1]], 1, backend="numpy")


# ---- size_buckets -----------------------------------------------------------


def _size_sets():
    rng = np.random.default_rng(2718)
    seeded = [(int(w), int(h)) for w, h in zip(rng.integers(1, 700, 200), rng.integers(1, 500, 200))]
    return {
        "seeded200": seeded,
        "all_equal": [(64, 48)] * 37,
        "one": [(5, 9)],
        "huge_and_tiny": [(4000, 3000)] + [(3, 2)] * 50,
        "nested": [(10 * k, 7 * k) for k in range(1, 40)],
        "empty": [],
    }


@pytest.mark.parametrize("batch_size", [None, 1, 5])
@pytest.mark.parametrize("min_fill", [0.5, 0.9, 0.0])
@pytest.mark.parametrize("name", list(_size_sets()))
def test_size_buckets(pconv_mod, name, min_fill, batch_size):
    from pconv.ops import stencil

    sizes = _size_sets()[name]
    for channels, fuse, max_bytes in (("rgb", 8, stencil._BATCH_BYTES), (1, 4, 1 << 22)):
        kw = dict(min_fill=min_fill, batch_size=batch_size, max_bytes=max_bytes)
        buckets = pconv_mod.size_buckets(sizes, channels, fuse, **kw)
        assert buckets == pconv_mod.size_buckets(list(sizes), channels, fuse, **kw)  # deterministic
        seen = [i for _, idx in buckets for i in idx]
        assert sorted(seen) == list(range(len(sizes)))  # a partition of the indices
        order = sorted(range(len(sizes)), key=lambda i: (-sizes[i][1], -sizes[i][0]))
        assert seen == order  # (height, width) descending, stable
        ch = {"rgb": "rgb", 1: "grey"}[channels]
        for (W, H), idx in buckets:
            assert len(idx) >= 1
            assert W == max(sizes[i][0] for i in idx) and H == max(sizes[i][1] for i in idx)
            if len(idx) > 1:
                fill = sum(sizes[i][0] * sizes[i][1] for i in idx) / (len(idx) * W * H)
                assert fill >= min_fill, (name, fill)
                assert 2 * len(idx) * stencil._frame_bytes(W, H, ch, fuse) <= max_bytes
            if batch_size is not None:
                assert len(idx) <= batch_size
    if name == "all_equal" and batch_size is None:
        assert len(pconv_mod.size_buckets(sizes, "rgb", 8, min_fill=min_fill)) == 1
    if name == "huge_and_tiny" and batch_size is None and min_fill == 0.5:
        b = pconv_mod.size_buckets(sizes, "rgb", 8)
        # the huge image shares its envelope with at most one tiny one (fill 0.5 + eps), the rest go together
        assert b[0][0] == (4000, 3000) and len(b[0][1]) <= 2 and len(b) == 2


def test_size_buckets_arguments(pconv_mod):
    # two images always reach fill 0.5: (64 + 16) / (2 * 64)
    assert pconv_mod.size_buckets([(4, 4), (8, 8)], "grey", lambda w, h: 8) == [((8, 8), [1, 0])]
    assert pconv_mod.size_buckets([(4, 4), (8, 8)], "grey", 8, min_fill=0.7) == [((8, 8), [1]), ((4, 4), [0])]
    with pytest.raises(ValueError, match="channels"):
        pconv_mod.size_buckets([(4, 4)], 2, 8)
    with pytest.raises(ValueError, match="1x1"):
        pconv_mod.size_buckets([(0, 4)], 1, 8)
    with pytest.raises(ValueError, match="min_fill"):
        pconv_mod.size_buckets([(4, 4)], 1, 8, min_fill=-0.1)
    with pytest.raises(ValueError, match="batch_size"):
        pconv_mod.size_buckets([(4, 4)], 1, 8, batch_size=0)
