"""Decimated results and pyramids on a real MI355X.

The decimation kernel on raw pointers at the output widths and heights where
its lanes, waves and workgroups end, for every pixel size, on both store paths,
with dirty source pads and canaries around and INSIDE the destination: the
output region equals ``img[first::s, ::s]`` and every other destination byte
keeps its canary.  Then the guards, the engines, the pyramid and the CLI, each
against the NumPy / CPU oracle.

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
PBS = [1, 2, 3, 4, 6, 8]
FACTORS = [2, 3, 4, 7, 16]
STORES = ["dword", "byte_offset", "byte_pitch"]
OUT_ROW_BYTES = [1, 3, 4, 5, 255, 256, 257, 1025]  # one lane, one wave (256 B) and one workgroup row around their edges


def _ceil(a, b):
    return -(-a // b)


def _src_frames(rng, pb, w, h, frames):
    """`frames` dirty source frames: one ghost row above and below and the pad
    columns hold 0xFF, the image rows random bytes.  Returns the images, the
    device buffer, (pitch, stride) and the offset of frame 0's (row 0, column 0)."""
    import torch

    rb = w * pb
    pitch = _ceil(16 + rb + 32, 128) * 128
    stride = (h + 2) * pitch
    full = np.full((frames, h + 2, pitch), DIRTY, np.uint8)
    imgs = rng.integers(0, 256, size=(frames, h, rb), dtype=np.uint8)
    full[:, 1:1 + h, 16:16 + rb] = imgs
    buf = torch.full((frames * stride + 2 * GUARD,), DIRTY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + frames * stride] = torch.from_numpy(full.reshape(-1)).cuda()
    return imgs, buf, pitch, stride, GUARD + pitch + 16


def _decimate_case(native, rng, pb, s, w, h, store, g_row0=0, frames=1, sizes=None):
    """One launch, checked byte for byte over the whole destination buffer.
    sizes: [(width, height)] per frame inside the w x h envelope (a dims table)."""
    import torch

    imgs, src, pitch, stride, src_off = _src_frames(rng, pb, w, h, frames)
    first = (s - g_row0 % s) % s
    out_h = _ceil(h - first, s) if h > first else 0
    out_rb = _ceil(w, s) * pb
    if store == "dword":
        off, dst_pitch = 0, _ceil(out_rb, 4) * 4 + 8
        dst_stride = max(out_h, 1) * dst_pitch + 12
    elif store == "byte_offset":
        off, dst_pitch = 1, _ceil(out_rb, 4) * 4 + 8
        dst_stride = max(out_h, 1) * dst_pitch + 12
    else:
        off, dst_pitch = 0, (out_rb | 1) + 2  # odd
        dst_stride = max(out_h, 1) * dst_pitch + 12
    dst_bytes = frames * dst_stride
    dst = torch.full((dst_bytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    expect = np.full(dst_bytes + 2 * GUARD, CANARY, np.uint8)
    for f in range(frames):
        fw, fh = sizes[f] if sizes else (w, h)
        keep = imgs[f, :fh, :fw * pb].reshape(fh, fw, pb)[first::s, ::s].reshape(-1, _ceil(fw, s) * pb)
        base = GUARD + off + f * dst_stride
        for y in range(keep.shape[0]):
            expect[base + y * dst_pitch: base + y * dst_pitch + keep.shape[1]] = keep[y]
    kw = {}
    if sizes:
        table = torch.tensor([[fw * pb, fh] for fw, fh in sizes], dtype=torch.int32, device="cuda")
        kw = dict(dims=[(fw * pb, fh) for fw, fh in sizes], dims_ptr=table.data_ptr())
    torch.cuda.synchronize()
    native.launch_decimate(src.data_ptr() + src_off, pitch, w * pb, h, dst.data_ptr() + GUARD + off, dst_pitch,
                           dst_bytes, pb, s, g_row0=g_row0, frames=frames, src_stride=stride,
                           dst_stride=dst_stride, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, (f"pb {pb} s {s} {w}x{h} {store} g_row0 {g_row0} frames {frames}: {bad.size} wrong bytes, "
                           f"first at {bad[:4] - GUARD}")


def _geometries(pb, s):
    """(W, H) pairs: output rows of about 1, 3, 4, 5, 255, 256, 257 and 1025
    bytes (the nearest whole pixel), output heights 1, 4, 5 and around the 16
    rows a workgroup covers; W and H no multiples of s, one pair of multiples,
    and a 3 x 2 image (s larger than both from 4 on)."""
    heights = [1, 4, 5, 15, 16, 17, 33, 2]
    geo = []
    for i, target in enumerate(OUT_ROW_BYTES):
        ow = max(1, round(target / pb))
        oh = heights[i % len(heights)]
        geo.append((ow * s - s // 2, oh * s - s // 2))
    geo.append((5 * s, 4 * s))
    geo.append((3, 2))
    return geo


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("s", FACTORS)
@pytest.mark.parametrize("pb", PBS)
def test_raw_kernel_output_and_canaries(native, pb, s, store):
    rng = np.random.default_rng(7919 * pb + 31 * s + len(store))
    for w, h in _geometries(pb, s):
        _decimate_case(native, rng, pb, s, w, h, store)


@pytest.mark.parametrize("s", FACTORS)
@pytest.mark.parametrize("pb", [1, 3, 6, 8])
def test_raw_kernel_band_phase(native, pb, s):
    """Selection by GLOBAL row: frame row r is kept when (g_row0 + r) % s == 0."""
    rng = np.random.default_rng(101 * pb + s)
    for g_row0 in (0, 1, s - 1, s + 1):
        for store in ("dword", "byte_pitch"):
            _decimate_case(native, rng, pb, s, 13, 2 * s + 3, store, g_row0=g_row0)
    # a band with no selected row writes nothing
    _decimate_case(native, rng, pb, s, 13, 1, "dword", g_row0=1)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("pb", PBS)
def test_raw_kernel_frames_and_dims(native, pb, store):
    rng = np.random.default_rng(53 * pb + len(store))
    _decimate_case(native, rng, pb, 3, 50, 37, store, frames=3)
    # mixed sizes in an envelope of two workgroups a row and three block rows:
    # a 1 x 1 image, one whose output ends inside the first workgroup, one whose
    # output ends inside the second workgroup of the row, and the whole envelope
    block = native.DECIMATE_BLOCK_ROWS
    w, h = 2 * (300 // pb + 1), 2 * (2 * block + 3)
    sizes = [(1, 1), (9, 7), (w - 5, h - 2 * block), (w, h)]
    _decimate_case(native, rng, pb, 2, w, h, store, frames=4, sizes=sizes)


@pytest.mark.parametrize("s", [1, 5])
def test_kernel_clamps_a_device_table_that_disagrees_with_its_host_copy(native, s):
    """The guards read the host list; the kernel reads the device table and
    clamps each entry to the envelope.  Entries beyond the envelope give
    exactly the envelope's output, entries below zero leave the frame alone.
    At both factors the 4 pixels and the one row more would each add to the
    output; unclamped they are read from frame 0's pad and ghost row and land
    in the destination's spare bytes and spare row, inside the buffers: a wrong
    kernel fails the comparison."""
    import torch

    rng = np.random.default_rng(977 + s)
    pb, w, h, frames = 4, 10, 5, 2
    rb = w * pb
    imgs, src, pitch, stride, src_off = _src_frames(rng, pb, w, h, frames)
    assert rb + 16 <= pitch - 16
    out_rb, out_h = _ceil(w, s) * pb, _ceil(h, s)
    assert _ceil(w + 4, s) * pb > out_rb and _ceil(h + 1, s) > out_h
    dst_pitch = _ceil(w + 4, s) * pb + 8
    dst_stride = (_ceil(h + 1, s) + 1) * dst_pitch
    dst = torch.full((frames * dst_stride + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    expect = np.full((frames, dst_stride // dst_pitch, dst_pitch), CANARY, np.uint8)
    expect[0, :out_h, :out_rb] = imgs[0].reshape(h, w, pb)[::s, ::s].reshape(out_h, out_rb)
    table = torch.tensor([[rb + 16, h + 1], [-1, -1]], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    native.launch_decimate(src.data_ptr() + src_off, pitch, rb, h, dst.data_ptr() + GUARD, dst_pitch,
                           frames * dst_stride, pb, s, frames=frames, src_stride=stride, dst_stride=dst_stride,
                           stream=torch.cuda.current_stream().cuda_stream, dims=[(rb, h), (rb, h)],
                           dims_ptr=table.data_ptr())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all(), "a canary outside the frames"
    got = got[GUARD:-GUARD].reshape(expect.shape)
    assert (got[1] == CANARY).all(), "frame 1 (a negative entry) was written"
    bad = np.argwhere(got[0] != expect[0])
    assert bad.size == 0, f"frame 0: {len(bad)} wrong bytes, first at (row, byte) {bad[:4].tolist()}"


def test_guards_refuse_and_write_nothing(native):
    import torch

    rng = np.random.default_rng(5)
    pb, w, h, s = 4, 20, 10, 2
    imgs, src, pitch, stride, src_off = _src_frames(rng, pb, w, h, 2)
    out_rb, out_h = _ceil(w, s) * pb, _ceil(h, s)
    dst_pitch, dst_stride = out_rb, out_rb * out_h
    dst = torch.full((2 * dst_stride + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[w * pb, h], [w * pb, h]], dtype=torch.int32, device="cuda")
    good = dict(src=src.data_ptr() + src_off, src_pitch=pitch, row_bytes=w * pb, rows=h,
                dst=dst.data_ptr() + GUARD, dst_pitch=dst_pitch, dst_bytes=2 * dst_stride, pixel_bytes=pb, factor=s,
                frames=2, src_stride=stride, dst_stride=dst_stride)
    bad = [
        (dict(factor=0), "factor"),
        (dict(factor=65), "factor"),
        (dict(pixel_bytes=5), "pixel_bytes"),
        (dict(pixel_bytes=3), "no whole pixels"),
        (dict(row_bytes=pitch + 4), "source pitch"),
        (dict(rows=0), "empty source frame"),
        (dict(g_row0=-1), "g_row0"),
        (dict(src=src.data_ptr() + src_off + 1), "multiples of 4"),
        (dict(dst_pitch=out_rb - 4), "destination pitch"),
        (dict(dst_bytes=2 * dst_stride - 1), "exceed dst_bytes"),
        (dict(frames=1, dst_bytes=dst_stride - 1), "exceeds dst_bytes"),
        (dict(dst_stride=dst_stride - 4), "frames would overlap"),
        (dict(src_stride=pitch), "frames would overlap"),
        (dict(frames=0), "frames must be"),
        (dict(dims=[(w * pb, h), (w * pb, h)]), "given together"),
        (dict(dims=[(w * pb, h), (w * pb + 4, h)], dims_ptr=table.data_ptr()), "dims[1].row_bytes"),
        (dict(dims=[(w * pb, h), (w * pb - 1, h)], dims_ptr=table.data_ptr()), "dims[1].row_bytes"),
        (dict(dims=[(w * pb, h + 1), (w * pb, h)], dims_ptr=table.data_ptr()), "dims[0].height"),
        (dict(dims=[(w * pb, h), (w * pb, h)], dims_ptr=table.data_ptr(), g_row0=2), "whole images"),
        (dict(active=[0, 1], active_ptr=table.data_ptr()), "active table is not supported"),
        (dict(rows=1 << 31, src_stride=(1 << 31) * pitch), "32-bit"),
    ]
    for change, text in bad:
        with pytest.raises(RuntimeError, match="launch_decimate: ") as err:
            native.launch_decimate(**{**good, **change})
        assert text in str(err.value), (change, str(err.value))
    torch.cuda.synchronize()
    assert bool((dst == CANARY).all()), "a refused launch wrote to the destination"
    # the grid limit (images x blocks < 2^31) needs no memory to be refused: 2^20 frames of 2^12 blocks
    with pytest.raises(RuntimeError, match="launch_decimate: too many workgroups"):
        big_rows = 4096 * native.DECIMATE_BLOCK_ROWS
        native.launch_decimate(**{**good, "rows": big_rows, "row_bytes": 4, "factor": 1, "frames": 1 << 20,
                                  "src_stride": big_rows * pitch, "dst_pitch": 4, "dst_stride": big_rows * 4,
                                  "dst_bytes": (1 << 20) * big_rows * 4})
    native.launch_decimate(**good)  # and the unchanged arguments do launch
    torch.cuda.synchronize()
    got = dst[GUARD:GUARD + 2 * dst_stride].cpu().numpy().reshape(2, out_h, out_rb)
    want = imgs.reshape(2, h, w, pb)[:, ::s, ::s].reshape(2, out_h, out_rb)
    assert np.array_equal(got, want)


# ---- engines ------------------------------------------------------------------

_ORACLE = {}


def _engine_image(depth):
    rng = np.random.default_rng(77 + depth)
    return rng.integers(0, 1 << depth, size=(61, 77, 3)).astype(np.uint8 if depth == 8 else np.uint16)


def _engine_oracle(pconv_mod, depth, border):
    key = (depth, border)
    if key not in _ORACLE:
        _ORACLE[key] = pconv_mod.numpy_convolve(_engine_image(depth), 21, "gaussian", border)
    return _ORACLE[key]


@pytest.mark.parametrize("border", ["zero", "replicate"])
@pytest.mark.parametrize("depth", [8, 16])
def test_engine_decimate(pconv_mod, depth, border):
    import torch

    img = _engine_image(depth)
    full = _engine_oracle(pconv_mod, depth, border)
    eng = pconv_mod.Engine(77, 61, "rgb", border=border, depth=depth)
    plain = eng(img, 21)
    assert np.array_equal(plain, full)
    one = eng(img, 21, decimate=1)
    assert one.dtype == plain.dtype and np.array_equal(one, plain), "decimate=1 differs from the plain call"
    for s in (2, 5):
        want = full[::s, ::s]
        got = eng(img, 21, decimate=s)
        assert isinstance(got, np.ndarray) and got.dtype == img.dtype and got.shape == want.shape
        assert np.array_equal(got, want), f"numpy in, s={s}"
        t = torch.from_numpy(img).cuda()
        got_t = eng(t, 21, decimate=s)
        assert got_t.is_cuda and got_t.dtype == t.dtype and tuple(got_t.shape) == want.shape
        assert np.array_equal(got_t.cpu().numpy(), want), f"CUDA tensor in, s={s}"
        assert np.array_equal(pconv_mod.convolve(t, 21, border=border, decimate=s).cpu().numpy(), want)


def test_batch_engine_decimate(pconv_mod):
    import torch

    rng = np.random.default_rng(4733)
    stack = rng.integers(0, 256, size=(3, 33, 47, 3), dtype=np.uint8)
    want = np.stack([pconv_mod.numpy_convolve(im, 9, "gaussian")[::2, ::2] for im in stack])
    eng = pconv_mod.BatchEngine(47, 33, "rgb", capacity=3)
    got = eng(stack, 9, decimate=2)
    assert got.shape == want.shape and np.array_equal(got, want)
    got_t = eng(torch.from_numpy(stack).cuda(), 9, decimate=2)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)
    assert np.array_equal(eng(stack[:2], 9, decimate=2), want[:2]), "n = 2 of 3"
    assert np.array_equal(eng(torch.from_numpy(stack[:2]).cuda(), 9, decimate=2).cpu().numpy(), want[:2])
    assert np.array_equal(eng(stack, 9, decimate=1), eng(stack, 9))
    assert np.array_equal(pconv_mod.convolve_batch(stack, 9, backend="hip", decimate=2), want)
    assert np.array_equal(pconv_mod.convolve_batch(stack, 9, backend="hip", decimate=2, batch_size=2), want)

    images = [rng.integers(0, 256, size=sh + (3,), dtype=np.uint8) for sh in [(40, 50), (1, 1), (37, 64)]]
    wants = [pconv_mod.numpy_convolve(im, 9, "gaussian")[::2, ::2] for im in images]
    env = pconv_mod.BatchEngine(64, 40, "rgb", capacity=3)
    for got, w in zip(env.run_images(images, 9, decimate=2), wants):
        assert got.shape == w.shape and np.array_equal(got, w)
    for got, w in zip(env.run_images([torch.from_numpy(im).cuda() for im in images], 9, decimate=2), wants):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), w)
    for got, w in zip(pconv_mod.convolve_many(images, 9, backend="hip", decimate=2), wants):
        assert got.shape == w.shape and np.array_equal(got, w)


@pytest.mark.parametrize("shape", [(61, 77, 3), (64, 64)])
def test_pyramid(pconv_mod, shape):
    import torch

    rng = np.random.default_rng(shape[0])
    h, w = shape[:2]
    ch = "rgb" if len(shape) == 3 else "grey"
    levels = len(pconv_mod.ops.pyramid_sizes(w, h))
    pyr = pconv_mod.Pyramid(w, h, ch, levels)
    assert len(pyr._engines) == levels - 1
    engines = list(pyr._engines)
    for call in range(2):  # the second call: other data through the same engines, no stale state
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        want = pconv_mod.pyramid(img, levels, backend="omp")
        assert want[-1].shape[:2] == (1, 1)
        got = pyr(img)
        got_t = pyr(torch.from_numpy(img).cuda())
        one_shot = pconv_mod.pyramid(img, levels, backend="hip")
        assert len(got) == len(got_t) == len(one_shot) == levels
        for k in range(levels):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (call, k)
            assert got_t[k].is_cuda and np.array_equal(got_t[k].cpu().numpy(), want[k]), (call, k)
            assert np.array_equal(one_shot[k], want[k]), (call, k)
    assert all(a is b for a, b in zip(engines, pyr._engines))


def test_cli_hip_decimate(tmp_path):
    out = tmp_path / "o.raw"
    p = subprocess.run([CONV_BIN, "x.raw", "77", "61", "9", "rgb", "--synthetic", "3", "--decimate", "2", "--frames",
                        "3", "--check", "--json", "--quiet", "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    js = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert js["mismatches"] == 0 and js["backend"] == "hip"
    assert (js["decimate"], js["out_width"], js["out_height"]) == (2, 39, 31)
    assert out.stat().st_size == 3 * 31 * 39 * 3
