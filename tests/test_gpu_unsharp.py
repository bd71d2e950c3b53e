"""The unsharp mask on a real MI355X.

The kernel on raw pointers: the original and the blurred frame are INDEPENDENT
random arrays with every boundary of the formula planted in them, so each
branch is reached whatever a blur would give.  Row bytes sit around one lane
(16 B) and one workgroup row (1024 B), heights around the rows a workgroup
covers, at both depths, out of place and in place, with dirty source pads and
ghost rows and canaries everywhere else: the WHOLE destination buffer is
compared byte for byte.  Then frames, a dims table, the guards, the engines
against ``numpy_unsharp`` and the CLI.

Exact bytes only."""
import json
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
DIRTY = 0xFF
ROW_BYTES = {8: [1, 15, 16, 17, 18, 1023, 1024, 1025, 1026], 16: [2, 14, 16, 18, 1022, 1024, 1026]}


def _pairs(depth):
    top = (1 << depth) - 1
    return [(1, 0), (16, 0), (255, 0), (24, top // 8), (16, top)]


def _ceil(a, b):
    return -(-a // b)


def _formula(x, b, k, t, top):
    """The issue's definition, restated: int64 arithmetic, floor shift."""
    x = x.astype(np.int64)
    b = b.astype(np.int64)
    sharp = np.clip((x * (16 + k) - b * k + 8) >> 4, 0, top)
    return np.where(np.abs(x - b) < t, x, sharp)


def _boundary_pairs(k, t, top):
    """(x, b) on every boundary: the extremes, |d| = t and t - 1 on both sides,
    and numerators of exactly -1, 0, 16 top + 15 and 16 top + 16 where a pair
    of samples gives one (x (16 + k) - b k + 8 is not onto for every k)."""
    pairs = [(0, top), (top, 0), (0, 0), (top, top)]
    for d in (t, t - 1):
        if 0 <= d <= top:
            pairs += [(d, 0), (0, d), (top, top - d), (top - d, top)]
    xs = np.arange(top + 1, dtype=np.int64)
    for target in (-1, 0, 16 * top + 15, 16 * top + 16):
        num = xs * (16 + k) + 8 - target  # = b k
        ok = (num % k == 0) & (num // k >= 0) & (num // k <= top)
        for x in xs[ok][:2]:
            pairs.append((int(x), int((x * (16 + k) + 8 - target) // k)))
    return pairs


def _samples(rng, depth, shape, k, t):
    """Independent random originals and blurred samples of `shape`, the
    boundary pairs planted at random places (as many as fit)."""
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    x = rng.integers(0, top + 1, size=shape).astype(dt)
    b = rng.integers(0, top + 1, size=shape).astype(dt)
    # half of the blurred samples near the original: both threshold branches are common
    near = rng.random(shape) < 0.5
    b = np.where(near, np.clip(x.astype(np.int64) + rng.integers(-40, 41, size=shape), 0, top), b).astype(dt)
    pairs = _boundary_pairs(k, t, top)
    n = x.size
    at = rng.permutation(n)[:len(pairs)]
    xf, bf = x.reshape(-1), b.reshape(-1)
    for i, (px, pb) in zip(at, pairs):
        xf[i], bf[i] = px, pb
    return x, b


def _frames(rows_of_bytes, rb, h, frames, fill):
    """`frames` pitched frames, one ghost row above and below, 16 pad bytes left:
    (full array (frames, h + 2, pitch) filled with `fill` around the rows, pitch)."""
    pitch = _ceil(16 + _ceil(rb, 16) * 16 + 32, 128) * 128
    full = np.full((frames, h + 2, pitch), fill, np.uint8)
    full[:, 1:1 + h, 16:16 + rb] = rows_of_bytes
    return full, pitch


def _device(full):
    """The frames between two guard regions of their own fill on the device."""
    import torch

    fill = int(full[0, 0, 0])
    buf = torch.full((full.size + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + full.size] = torch.from_numpy(full.reshape(-1)).cuda()
    return buf


def _unsharp_case(native, rng, depth, k, t, rb, h, in_place, frames=1, dims=None):
    """One launch, the whole destination buffer checked byte for byte.
    dims: [(row_bytes, height)] per frame inside the rb x h envelope."""
    import torch

    sb, top = depth // 8, (1 << depth) - 1
    x, b = _samples(rng, depth, (frames, h, rb // sb), k, t)
    xo, pitch = _frames(x.view(np.uint8).reshape(frames, h, rb), rb, h, frames, DIRTY)
    xb, _ = _frames(b.view(np.uint8).reshape(frames, h, rb), rb, h, frames, DIRTY)
    orig, blur = _device(xo), _device(xb)
    if in_place:
        dst, expect = blur, xb.copy()
    else:
        expect = np.full_like(xb, CANARY)
        dst = _device(expect)
    want = _formula(x, b, k, t, top).astype(x.dtype).view(np.uint8).reshape(frames, h, rb)
    for f in range(frames):
        frb, fh = dims[f] if dims else (rb, h)
        expect[f, 1:1 + fh, 16:16 + frb] = want[f, :fh, :frb]
    kw = {}
    if dims:
        table = torch.tensor(dims, dtype=torch.int32, device="cuda")
        kw = dict(dims=list(dims), dims_ptr=table.data_ptr())
    off, stride = GUARD + pitch + 16, (h + 2) * pitch
    torch.cuda.synchronize()
    native.launch_unsharp(orig.data_ptr() + off, pitch, blur.data_ptr() + off, pitch, dst.data_ptr() + off, pitch, rb,
                          h, depth=depth, k=k, threshold=t, frames=frames, orig_stride=stride, blur_stride=stride,
                          dst_stride=stride, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    fill = DIRTY if in_place else CANARY
    whole = np.concatenate([np.full(GUARD, fill, np.uint8), expect.reshape(-1), np.full(GUARD, fill, np.uint8)])
    bad = np.flatnonzero(got != whole)
    assert bad.size == 0, (f"depth {depth} k {k} t {t} {rb} B x {h} rows in_place {in_place} frames {frames}: "
                           f"{bad.size} wrong bytes, first at {bad[:4] - GUARD}")
    # the sources are only read
    assert np.array_equal(orig.cpu().numpy()[GUARD:-GUARD], xo.reshape(-1))
    if not in_place:
        assert np.array_equal(blur.cpu().numpy()[GUARD:-GUARD], xb.reshape(-1))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("pair", range(5))
@pytest.mark.parametrize("depth", [8, 16])
def test_raw_kernel_output_and_canaries(native, depth, pair, in_place):
    k, t = _pairs(depth)[pair]
    rng = np.random.default_rng(7919 * depth + 31 * pair + in_place)
    block = native.UNSHARP_BLOCK_ROWS
    for rb in ROW_BYTES[depth]:
        for h in (1, block - 1, block, block + 1, 2 * block + 1):
            _unsharp_case(native, rng, depth, k, t, rb, h, in_place)


def test_planted_pairs_reach_every_branch():
    """The planted data itself: for (24, max // 8) it clamps at 0, at max, keeps
    and changes samples at both depths, and the numerators asked for occur."""
    for depth in (8, 16):
        top = (1 << depth) - 1
        k, t = 24, top // 8
        x, b = _samples(np.random.default_rng(3), depth, (1, 17, 600), k, t)
        xi, bi = x.astype(np.int64), b.astype(np.int64)
        num = xi * (16 + k) - bi * k + 8
        out = _formula(x, b, k, t, top)
        live = np.abs(xi - bi) >= t
        assert (live & (num < 0)).any() and (live & (num >= 16 * (top + 1))).any()
        assert (~live).any() and (out != xi).any()
        assert (np.abs(xi - bi) == t).any() and (np.abs(xi - bi) == t - 1).any()
        k1 = _boundary_pairs(1, 0, top)
        nums = {px * 17 - pb + 8 for px, pb in k1}
        assert {-1, 0, 16 * top + 15, 16 * top + 16} <= nums


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("depth", [8, 16])
def test_raw_kernel_frames_and_dims(native, depth, in_place):
    rng = np.random.default_rng(53 * depth + in_place)
    sb, top = depth // 8, (1 << depth) - 1
    _unsharp_case(native, rng, depth, 24, top // 8, 150, 37, in_place, frames=3)
    # mixed sizes in an envelope of two workgroups a row and three block rows: a
    # 1 x 1 image, one that ends inside the first workgroup, one that ends inside
    # the second workgroup of the row (and of the column), and the whole envelope
    block = native.UNSHARP_BLOCK_ROWS
    rb, h = 1024 + 300, 2 * block + 3
    dims = [(sb, 1), (18, 7), (1024 + 102, block + 5), (rb, h)]
    _unsharp_case(native, rng, depth, 24, top // 8, rb, h, in_place, frames=4, dims=dims)


def test_kernel_clamps_a_device_table_that_disagrees_with_its_host_copy(native):
    """The guards read the host list; the kernel reads the device table and
    clamps each entry to the envelope.  Entries beyond the envelope give
    exactly the envelope, entries below zero leave the frame alone.  (Unclamped,
    the 16 bytes and the one row more would land in frame 0's pad and ghost row,
    inside the buffer: a wrong kernel fails the comparison.)"""
    import torch

    rng = np.random.default_rng(977)
    rb, h, frames, k, t = 40, 5, 2, 24, 31
    x, b = _samples(rng, 8, (frames, h, rb), k, t)
    xo, pitch = _frames(x, rb, h, frames, DIRTY)
    xb, _ = _frames(b, rb, h, frames, DIRTY)
    assert rb + 16 <= pitch - 16
    expect = np.full_like(xb, CANARY)
    expect[0, 1:1 + h, 16:16 + rb] = _formula(x[0], b[0], k, t, 255).astype(np.uint8)
    orig, blur, dst = _device(xo), _device(xb), _device(np.full_like(xb, CANARY))
    table = torch.tensor([[rb + 16, h + 1], [-1, -1]], dtype=torch.int32, device="cuda")
    off, stride = GUARD + pitch + 16, (h + 2) * pitch
    torch.cuda.synchronize()
    native.launch_unsharp(orig.data_ptr() + off, pitch, blur.data_ptr() + off, pitch, dst.data_ptr() + off, pitch, rb,
                          h, depth=8, k=k, threshold=t, frames=frames, orig_stride=stride, blur_stride=stride,
                          dst_stride=stride, stream=torch.cuda.current_stream().cuda_stream,
                          dims=[(rb, h), (rb, h)], dims_ptr=table.data_ptr())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all(), "a canary outside the frames"
    got = got[GUARD:-GUARD].reshape(expect.shape)
    assert np.array_equal(got[1], expect[1]), "frame 1 (a negative entry) was written"
    bad = np.argwhere(got[0] != expect[0])
    assert bad.size == 0, f"frame 0: {len(bad)} wrong bytes, first at (row, byte) {bad[:4].tolist()}"
    assert np.array_equal(orig.cpu().numpy()[GUARD:-GUARD], xo.reshape(-1))
    assert np.array_equal(blur.cpu().numpy()[GUARD:-GUARD], xb.reshape(-1))


def test_guards_refuse_and_write_nothing(native):
    import torch

    rng = np.random.default_rng(5)
    rb, h, frames = 80, 10, 2
    x, b = _samples(rng, 8, (frames, h, rb), 16, 0)
    xo, pitch = _frames(x, rb, h, frames, DIRTY)
    xb, _ = _frames(b, rb, h, frames, DIRTY)
    canaries = np.full_like(xb, CANARY)
    orig, blur, dst = _device(xo), _device(xb), _device(canaries)
    off, stride = GUARD + pitch + 16, (h + 2) * pitch
    table = torch.tensor([[rb, h], [rb, h]], dtype=torch.int32, device="cuda")
    good = dict(orig=orig.data_ptr() + off, orig_pitch=pitch, blur=blur.data_ptr() + off, blur_pitch=pitch,
                dst=dst.data_ptr() + off, dst_pitch=pitch, row_bytes=rb, rows=h, depth=8, k=16, threshold=0,
                frames=frames, orig_stride=stride, blur_stride=stride, dst_stride=stride)
    bad = [
        (dict(depth=12), "depth"),
        (dict(k=0), "k 0"),
        (dict(k=256), "k 256"),
        (dict(threshold=-1), "threshold"),
        (dict(threshold=256), "threshold"),
        (dict(depth=16, row_bytes=rb - 1), "no whole samples"),
        (dict(rows=0), "empty frame"),
        (dict(row_bytes=0), "empty frame"),
        (dict(frames=0), "frames must be"),
        (dict(orig=0), "null frame pointer"),
        (dict(orig=orig.data_ptr() + off + 4), "multiple of 16"),
        (dict(blur=blur.data_ptr() + off + 8), "multiple of 16"),
        (dict(dst=dst.data_ptr() + off + 1), "multiple of 16"),
        (dict(dst_pitch=pitch + 8), "multiple of 16"),
        (dict(orig_stride=stride + 4), "multiple of 16"),
        (dict(row_bytes=pitch + 1), "rounded up to 16"),
        (dict(blur_pitch=64), "rounded up to 16"),
        (dict(dst_stride=pitch), "frames would overlap"),
        (dict(orig_stride=(h - 1) * pitch), "frames would overlap"),
        (dict(dims=[(rb, h), (rb, h)]), "given together"),
        (dict(dims=[(rb, h), (rb + 1, h)], dims_ptr=table.data_ptr()), "dims[1].row_bytes"),
        (dict(dims=[(rb, h), (0, h)], dims_ptr=table.data_ptr()), "dims[1].row_bytes"),
        (dict(depth=16, dims=[(rb, h), (rb - 1, h)], dims_ptr=table.data_ptr()), "dims[1].row_bytes"),
        (dict(dims=[(rb, h + 1), (rb, h)], dims_ptr=table.data_ptr()), "dims[0].height"),
        (dict(dims=[(rb, 0), (rb, h)], dims_ptr=table.data_ptr()), "dims[0].height"),
        (dict(active=[0, 1], active_ptr=table.data_ptr()), "active table is not supported"),
        (dict(rows=1 << 31), "32-bit"),
        (dict(dst=orig.data_ptr() + off), "dst overlaps orig"),
        (dict(dst=blur.data_ptr() + off + pitch), "dst overlaps blur"),
        (dict(dst=blur.data_ptr() + off, dst_pitch=2 * pitch, dst_stride=2 * stride), "dst overlaps blur"),
        (dict(dst=blur.data_ptr() + off, dst_stride=2 * stride), "dst overlaps blur"),
    ]
    for change, text in bad:
        with pytest.raises(RuntimeError, match="launch_unsharp: ") as err:
            native.launch_unsharp(**{**good, **change})
        assert text in str(err.value), (change, str(err.value))
    # the grid limit (images x blocks < 2^31) needs no memory to be refused: 2^20 frames of 2^12 blocks
    big_rows = 4096 * native.UNSHARP_BLOCK_ROWS
    with pytest.raises(RuntimeError, match="launch_unsharp: too many workgroups"):
        native.launch_unsharp(**{**good, "rows": big_rows, "frames": 1 << 20, "orig_stride": big_rows * pitch,
                                 "blur_stride": big_rows * pitch, "dst_stride": big_rows * pitch})
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all()), "a refused launch wrote to the destination"
    assert np.array_equal(blur.cpu().numpy()[GUARD:-GUARD], xb.reshape(-1)), "a refused launch wrote to blur"
    native.launch_unsharp(**good)  # and the unchanged arguments do launch
    torch.cuda.synchronize()
    got = dst.cpu().numpy()[GUARD:-GUARD].reshape(frames, h + 2, pitch)[:, 1:1 + h, 16:16 + rb]
    assert np.array_equal(got, _formula(x, b, 16, 0, 255).astype(np.uint8))


# ---- engines ------------------------------------------------------------------

_ORACLE = {}
REPS = 9


def _engine_image(depth, seed=0):
    rng = np.random.default_rng(77 + depth + 1000 * seed)
    return rng.integers(0, 1 << depth, size=(61, 77, 3)).astype(np.uint8 if depth == 8 else np.uint16)


def _engine_oracle(pconv_mod, depth, border, seed=0):
    """numpy_unsharp(image, REPS, 1.5, max // 64), computed once per case."""
    key = (depth, border, seed)
    if key not in _ORACLE:
        t = ((1 << depth) - 1) // 64
        _ORACLE[key] = pconv_mod.numpy_unsharp(_engine_image(depth, seed), REPS, 1.5, t, "gaussian", border)
    return _ORACLE[key]


@pytest.mark.parametrize("border", ["zero", "replicate"])
@pytest.mark.parametrize("depth", [8, 16])
def test_engine_unsharp(pconv_mod, depth, border):
    import torch

    t = ((1 << depth) - 1) // 64
    eng = pconv_mod.Engine(77, 61, "rgb", border=border, depth=depth)
    for seed in (0, 1):  # the second call: another image through the same engine, no stale original
        img = _engine_image(depth, seed)
        want = _engine_oracle(pconv_mod, depth, border, seed)
        got = eng.unsharp(img, REPS, 1.5, t)
        assert isinstance(got, np.ndarray) and got.dtype == img.dtype and got.shape == img.shape
        assert np.array_equal(got, want), f"numpy in, image {seed}"
        dev = torch.from_numpy(img).cuda()
        got_t = eng.unsharp(dev, REPS, 1.5, t)
        assert got_t.is_cuda and got_t.device == dev.device and got_t.dtype == dev.dtype
        assert np.array_equal(got_t.cpu().numpy(), want), f"CUDA tensor in, image {seed}"
        assert np.array_equal(dev.cpu().numpy(), img), "the input tensor was modified"
        cpu_t = eng.unsharp(torch.from_numpy(img), REPS, 1.5, t)
        assert not cpu_t.is_cuda and cpu_t.dtype == dev.dtype and np.array_equal(cpu_t.numpy(), want)
    img = _engine_image(depth, 0)
    # the plain call after an unsharp call: no sharpening left behind
    assert np.array_equal(eng(img, REPS), pconv_mod.numpy_convolve(img, REPS, "gaussian", border))
    assert np.array_equal(eng.unsharp(img, 0, 1.5, t), img), "reps = 0 returns the input"
    assert np.array_equal(pconv_mod.unsharp(img, REPS, 1.5, t, backend="hip", border=border),
                          _engine_oracle(pconv_mod, depth, border, 0))
    dev = torch.from_numpy(img).cuda()
    auto = pconv_mod.unsharp(dev, REPS, 1.5, t, border=border)  # auto: a CUDA tensor runs on hip
    assert auto.is_cuda and np.array_equal(auto.cpu().numpy(), _engine_oracle(pconv_mod, depth, border, 0))


def test_engine_refusals(pconv_mod, native):
    img = _engine_image(8)
    eng = pconv_mod.Engine(77, 61, "rgb")
    with pytest.raises(ValueError, match="unsharp amount must be a multiple of 1/16"):
        eng.unsharp(img, 3, 0.03)
    with pytest.raises(ValueError, match="unsharp threshold must be an integer"):
        eng.unsharp(img, 3, 1.0, 256)
    with pytest.raises(ValueError, match="per-channel amounts"):
        eng.unsharp(img, 3, (1.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="hipGraph capture"):
        pconv_mod.Engine(77, 61, "rgb", graph=True).unsharp(img, 3)
    with pytest.raises(RuntimeError, match="apply_unsharp: no original"):
        eng._eng.apply_unsharp(16, 0)
    with pytest.raises(ValueError, match="gaussian filter only"):
        pconv_mod.unsharp(_engine_image(16), 3, filter="box", backend="hip")


def test_batch_engine_unsharp(pconv_mod):
    import torch

    rng = np.random.default_rng(4733)
    stack = rng.integers(0, 256, size=(3, 33, 47, 3), dtype=np.uint8)
    want = np.stack([pconv_mod.numpy_unsharp(im, REPS, 1.5, 3) for im in stack])
    eng = pconv_mod.BatchEngine(47, 33, "rgb", capacity=3)
    got = eng.unsharp(stack, REPS, 1.5, 3)
    assert got.dtype == stack.dtype and got.shape == want.shape and np.array_equal(got, want)
    got_t = eng.unsharp(torch.from_numpy(stack).cuda(), REPS, 1.5, 3)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)
    assert np.array_equal(eng.unsharp(stack[:2][::-1], REPS, 1.5, 3), want[:2][::-1]), "n = 2 of 3, other images"
    assert np.array_equal(eng(stack, REPS), np.stack([pconv_mod.numpy_convolve(im, REPS) for im in stack]))
    assert np.array_equal(pconv_mod.unsharp_batch(stack, REPS, 1.5, 3, backend="hip"), want)
    assert np.array_equal(pconv_mod.unsharp_batch(stack, REPS, 1.5, 3, backend="hip", batch_size=2), want)
    with pytest.raises(RuntimeError, match="the snapshot holds 0"):
        eng._eng.apply_unsharp(16, 0, 3)

    images = [rng.integers(0, 256, size=sh + (3,), dtype=np.uint8) for sh in [(40, 50), (1, 1), (37, 64)]]
    wants = [pconv_mod.numpy_unsharp(im, REPS, 1.5, 3) for im in images]
    env = pconv_mod.BatchEngine(64, 40, "rgb", capacity=3)
    for got, w in zip(env.unsharp_images(images, REPS, 1.5, 3), wants):
        assert got.shape == w.shape and np.array_equal(got, w)
    for got, w in zip(env.unsharp_images([torch.from_numpy(im).cuda() for im in images], REPS, 1.5, 3), wants):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), w)
    for got, w in zip(pconv_mod.unsharp_many(images, REPS, 1.5, 3, backend="hip"), wants):
        assert got.shape == w.shape and np.array_equal(got, w)
    # depth 16 through the batch engine
    stack16 = rng.integers(0, 65536, size=(2, 21, 35, 3)).astype(np.uint16)
    want16 = np.stack([pconv_mod.numpy_unsharp(im, 4, 2.0, 1000) for im in stack16])
    assert np.array_equal(pconv_mod.unsharp_batch(stack16, 4, 2.0, 1000, backend="hip"), want16)


def test_cli_hip_unsharp(tmp_path):
    out = tmp_path / "o.raw"
    p = subprocess.run([CONV_BIN, "x.raw", "77", "61", "9", "rgb", "--synthetic", "3", "--unsharp", "1.5",
                        "--unsharp-threshold", "3", "--frames", "2", "--check", "--json", "--quiet", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    js = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["mismatches"] == 0 and js["backend"] == "hip"
    assert (js["unsharp"], js["unsharp_threshold"]) == (1.5, 3)
    assert out.stat().st_size == 2 * 61 * 77 * 3
