"""Depth 16 without a GPU: the NumPy oracle on uint16 against a brute-force
loop, the cpu / omp backends against the oracle, cpu_fused_launch(depth=16) on
band frames against stepwise numpy_step, the cross-depth property that ties
depth 16 to every 8-bit oracle, saturation, byte order, the named errors and
the CLI's --depth 16 (file round trip, size check, usage errors)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN, PKG

BORDERS = ["zero", "replicate"]
SIZES = [(1, 1), (1, 5), (5, 1), (3, 3), (2, 16), (17, 16), (31, 100), (64, 65)]
CH = {"grey": 1, "rgb": 3, "rgba": 4}


def _img(rng, h, w, c):
    a = rng.integers(0, 65536, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint16)
    a[h // 3:h // 3 + 2, w // 4:w // 4 + 5] = 65535  # a saturated block
    return a


def _brute(img, border):
    """One repetition, pixel by pixel, in Python integers."""
    x = img if img.ndim == 3 else img[:, :, None]
    h, w, c = x.shape
    k = (1, 2, 1)
    out = np.zeros_like(x)
    for y in range(h):
        for xx in range(w):
            for ch in range(c):
                acc = 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xc = y + dy, xx + dx
                        if border == "replicate":
                            yy, xc = min(max(yy, 0), h - 1), min(max(xc, 0), w - 1)
                        elif not (0 <= yy < h and 0 <= xc < w):
                            continue
                        acc += k[dy + 1] * k[dx + 1] * int(x[yy, xc, ch])
                out[y, xx, ch] = acc >> 4
    return out.reshape(img.shape)


@pytest.mark.parametrize("border", BORDERS)
def test_numpy_oracle_against_brute_force(pconv_mod, rng, border):
    for (h, w, c) in [(1, 1, 1), (1, 4, 3), (4, 1, 4), (5, 7, 1), (6, 5, 3)]:
        img = _img(rng, h, w, c)
        want = img
        for reps in (1, 2, 3):
            want = _brute(want, border)
            got = pconv_mod.numpy_convolve(img, reps, "gaussian", border)
            assert got.dtype == np.uint16 and np.array_equal(got, want), (h, w, c, reps)


def test_float32_formula_equals_the_integer_one(rng):
    """The reference's trunc(sum fl(p w / 16)) in float32, multiply then add in
    tap order, on full-range 16-bit samples: what makes depth 16 integer
    arithmetic on every backend."""
    from pconv.ops.reference import numpy_step

    img = _img(rng, 40, 60, 1)
    w32 = (np.array([1, 2, 1, 2, 4, 2, 1, 2, 1], np.float64) / 16.0).astype(np.float32).reshape(3, 3)
    x = img
    for _ in range(3):
        p = np.pad(x, 1)
        acc = np.zeros(x.shape, np.float32)
        for k in range(3):
            for l in range(3):
                acc = (acc + p[k:k + 40, l:l + 60].astype(np.float32) * w32[k, l]).astype(np.float32)
        f = np.trunc(acc).astype(np.uint16)
        x = numpy_step(x)
        assert np.array_equal(f, x)


@pytest.mark.parametrize("backend", ["cpu", "omp"])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
def test_cpu_backends_equal_the_oracle(pconv_mod, rng, channels, border, backend):
    for (h, w) in SIZES:
        img = _img(rng, h, w, CH[channels])
        for reps in (1, 2, 7):
            got = pconv_mod.convolve(img, reps, backend=backend, border=border)
            assert got.dtype == np.uint16 and got.shape == img.shape
            assert np.array_equal(got, pconv_mod.numpy_convolve(img, reps, "gaussian", border)), (h, w, reps)


def test_tensor_in_tensor_out(pconv_mod, rng):
    import torch

    img = _img(rng, 17, 16, 3)
    t = torch.from_numpy(img)
    out = pconv_mod.convolve(t, 3, backend="cpu")
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint16
    assert np.array_equal(out.numpy(), pconv_mod.numpy_convolve(img, 3))
    stack = np.stack([_img(rng, 9, 11, 3) for _ in range(3)])
    outs = pconv_mod.convolve_batch(stack, 4, backend="omp", border="replicate")
    assert outs.dtype == np.uint16
    for o, x in zip(outs, stack):
        assert np.array_equal(o, pconv_mod.numpy_convolve(x, 4, border="replicate"))
    many = pconv_mod.convolve_many([stack[0], stack[1][:5, :6]], 2, backend="cpu")
    assert np.array_equal(many[1], pconv_mod.numpy_convolve(np.ascontiguousarray(stack[1][:5, :6]), 2))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("steps", [1, 2, 5])
def test_cpu_fused_launch_on_band_frames(native, rng, border, steps):
    """g_row0 at, above and below the image edges; against stepwise numpy_step
    of the whole image."""
    from pconv.ops.reference import numpy_step

    H, w, c, h, halo = 40, 13, 3, 12, 5
    rb = w * c * 2
    img = _img(rng, H, w, c)
    ref = img
    for _ in range(steps):
        ref = numpy_step(ref, "gaussian", border)
    ref8 = ref.view(np.uint8).reshape(H, rb)
    lay = native.frame_layout(rb, h, halo)
    for g_row0 in (0, 14, H - h, -3, H - h + 4):
        src = np.zeros((h + 2 * halo, lay["pitch"]), np.uint8)
        for fr in range(-halo, h + halo):
            if 0 <= g_row0 + fr < H:
                src[halo + fr, 16:16 + rb] = img[g_row0 + fr].view(np.uint8).reshape(-1)
            elif border == "replicate":
                src[halo + fr, 16:16 + rb] = 0xEE  # never read under replicate
        for (r0, r1) in [(0, h), (-(halo - steps), h + halo - steps), (2, 3)]:
            dst = np.full_like(src, 0x77)
            native.cpu_fused_launch("gaussian", "rgb", rb, h, halo, src.reshape(-1), dst.reshape(-1), r0, r1, steps,
                                    g_row0, H, border=border, depth=16)
            for fr in range(r0, r1):
                g = g_row0 + fr
                if 0 <= g < H:
                    assert np.array_equal(dst[halo + fr, 16:16 + rb], ref8[g]), (g_row0, r0, r1, fr)
            assert (dst[:, :16] == 0x77).all() and (dst[:, 16 + rb:] == 0x77).all()
            assert (dst[:halo + r0] == 0x77).all() and (dst[halo + r1:] == 0x77).all()
    with pytest.raises(RuntimeError, match="depth 16 runs the gaussian filter only"):
        native.cpu_fused_launch("box", "rgb", rb, h, halo, src.reshape(-1), dst.reshape(-1), 0, h, 1, 0, H, depth=16)


@pytest.mark.parametrize("backend", ["numpy", "cpu", "omp"])
@pytest.mark.parametrize("border", BORDERS)
def test_cross_depth_property(pconv_mod, rng, border, backend):
    """convolve(x.astype(uint16)) == convolve(x).astype(uint16) for a uint8
    image: depth 16 agrees with every existing 8-bit oracle."""
    for shape in [(1, 1), (9, 14), (23, 31, 3), (16, 16, 4)]:
        x = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for r in (1, 6):
            a = pconv_mod.convolve(x.astype(np.uint16), r, backend=backend, border=border)
            b = pconv_mod.convolve(x, r, backend=backend, border=border)
            assert a.dtype == np.uint16 and b.dtype == np.uint8
            assert np.array_equal(a, b.astype(np.uint16)), (shape, r)


@pytest.mark.parametrize("backend", ["numpy", "cpu", "omp"])
def test_saturation_and_byte_order(pconv_mod, backend):
    full = np.full((9, 11, 3), 65535, np.uint16)
    assert (pconv_mod.convolve(full, 20, backend=backend, border="replicate") == 65535).all()
    # under the zero border the interior of one repetition stays saturated, the corner is 9/16
    one = pconv_mod.convolve(full, 1, backend=backend)
    assert (one[1:-1, 1:-1] == 65535).all() and one[0, 0, 0] == (9 * 65535) >> 4
    # 0x00FF / 0xFF00 alternating: a backend that swapped or dropped bytes differs
    pat = np.where(np.arange(8 * 10).reshape(8, 10) & 1, 0xFF00, 0x00FF).astype(np.uint16)
    want = pat
    for _ in range(2):
        want = _brute(want, "zero")
    assert np.array_equal(pconv_mod.convolve(pat, 2, backend=backend), want)


def test_other_dtypes_are_treated_as_before(pconv_mod, rng):
    x = rng.integers(0, 256, size=(7, 9), dtype=np.int32)
    out = pconv_mod.convolve(x, 2, backend="cpu")
    assert out.dtype == np.uint8 and np.array_equal(out, pconv_mod.numpy_convolve(x.astype(np.uint8), 2))


def test_named_errors(pconv_mod, rng):
    import torch

    img = _img(rng, 6, 7, 1)
    for backend in ("numpy", "cpu", "omp"):
        with pytest.raises(ValueError, match="gaussian filter only"):
            pconv_mod.convolve(img, 1, "box", backend=backend)
        with pytest.raises(ValueError, match="depth 16"):
            pconv_mod.convolve_until_stable(img, 4, backend=backend)
        with pytest.raises(ValueError, match="depth 16"):
            pconv_mod.residual(img, backend=backend)
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.convolve_batch_until_stable(img[None], 4, backend="cpu")
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.convolve_many_until_stable([img], 4, backend="cpu")
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.FilterPipeline.from_spec("gaussian:2").apply(img, backend="cpu")
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.numpy_residual(img)
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.convolve_until_stable(torch.from_numpy(img), 4, backend="cpu")
    from pconv.parallel.cpu_dist import local_cpu_cluster_convolve

    with pytest.raises(ValueError, match="depth 16"):
        local_cpu_cluster_convolve(img, 1, 2)
    with pytest.raises(RuntimeError, match="depth must be 8 or 16"):
        pconv_mod.native.cpu_convolve(img.view(np.uint8).reshape(-1), np.empty(img.size * 2, np.uint8), 7, 6, "grey", 1,
                                      depth=12)


def test_raw_io_and_size_buckets(pconv_mod, tmp_path):
    from pconv.ops.stencil import _frame_bytes, size_buckets

    a = pconv_mod.synthetic_image(13, 9, "rgb", seed=5, depth=16)
    assert a.dtype == np.uint16 and a.shape == (9, 13, 3)
    # the byte generator over the twice-as-wide row: identical for any band split
    b = np.concatenate([pconv_mod.synthetic_image(13, 9, "rgb", seed=5, y0=0, rows=4, depth=16),
                        pconv_mod.synthetic_image(13, 9, "rgb", seed=5, y0=4, rows=5, depth=16)])
    assert np.array_equal(a, b)
    p = str(tmp_path / "x.raw")
    pconv_mod.write_raw(p, a)
    assert os.path.getsize(p) == 13 * 9 * 3 * 2
    assert np.array_equal(np.fromfile(p, dtype="<u2").reshape(a.shape), a)
    assert np.array_equal(pconv_mod.read_raw(p, 13, 9, "rgb", depth=16), a)
    assert _frame_bytes(100, 10, "rgb", 8, depth=16) > _frame_bytes(100, 10, "rgb", 8)
    assert _frame_bytes(100, 10, "rgb", 8, depth=16) == _frame_bytes(200, 10, "rgb", 8)
    sizes = [(1000, 1000)] * 4
    n8 = len(size_buckets(sizes, "grey", 8, max_bytes=5 << 20))
    n16 = len(size_buckets(sizes, "grey", 8, max_bytes=5 << 20, depth=16))
    assert n16 > n8


# ---- CLI ----------------------------------------------------------------------

def _conv(tmp_path, *args):
    return subprocess.run([CONV_BIN, *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_cli_file_round_trip(pconv_mod, rng, tmp_path, backend):
    img = _img(rng, 19, 23, 3)
    img.astype("<u2").tofile(tmp_path / "in.raw")
    r = _conv(tmp_path, "in.raw", "23", "19", "4", "rgb", "--depth", "16", "--backend", backend, "--border",
              "replicate", "--out", "out.raw", "--check", "--json", "--quiet")
    assert r.returncode == 0, r.stderr
    import json

    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["depth"] == 16 and js["mismatches"] == 0
    want = pconv_mod.numpy_convolve(img, 4, "gaussian", "replicate").astype("<u2").tobytes()
    assert (tmp_path / "out.raw").read_bytes() == want
    # frames: two images back to back
    np.concatenate([img, img[::-1]]).astype("<u2").tofile(tmp_path / "two.raw")
    r = _conv(tmp_path, "two.raw", "23", "19", "2", "rgb", "--depth", "16", "--backend", backend, "--frames", "2",
              "--out", "two_out.raw", "--quiet")
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "two_out.raw", dtype="<u2").reshape(2, 19, 23, 3)
    assert np.array_equal(out[0], pconv_mod.numpy_convolve(img, 2))
    assert np.array_equal(out[1], pconv_mod.numpy_convolve(np.ascontiguousarray(img[::-1]), 2))


def test_cli_file_size_is_checked_with_the_depth(rng, tmp_path):
    rng.integers(0, 256, size=23 * 19 * 3, dtype=np.uint8).tofile(tmp_path / "eight.raw")  # an 8-bit file
    r = _conv(tmp_path, "eight.raw", "23", "19", "1", "rgb", "--depth", "16", "--backend", "cpu", "--quiet")
    assert r.returncode != 0 and "eight.raw" in r.stderr
    r = _conv(tmp_path, "eight.raw", "23", "19", "1", "rgb", "--backend", "cpu", "--quiet")
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("extra,what", [
    (["--filter", "box"], "--filter box"),
    (["--filter", "edge"], "--filter edge"),
    (["--gpus", "2"], "--gpus above 1"),
    (["--server", "/tmp/nowhere.sock"], "--server"),
    (["--bench", "3"], "--bench"),
    (["--backend", "auto"], "--backend auto"),
    (["--converge-every", "4"], "--converge-every"),
    (["--checkpoint-every", "4"], "--checkpoint-every"),
    (["--graph"], "--graph"),
    (["--kernel", "binomial"], "--kernel other than auto|temporal"),
    (["--kernel", "float_temporal"], "--kernel other than auto|temporal"),
])
def test_cli_usage_errors(tmp_path, extra, what):
    r = _conv(tmp_path, "s.raw", "8", "8", "1", "grey", "--depth", "16", "--synthetic", "1", *extra)
    assert r.returncode != 0
    assert "--depth 16 cannot be combined with " + what in r.stderr, r.stderr
    assert not (tmp_path / "blur_s.raw").exists()


def test_cli_rejects_other_depths(tmp_path):
    r = _conv(tmp_path, "s.raw", "8", "8", "1", "grey", "--depth", "12", "--synthetic", "1")
    assert r.returncode != 0 and "invalid --depth '12'" in r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_depth16_native_runner_asan_ubsan():
    """tests/cpp/test_depth16_native.cpp: the 16-bit row kernels and
    cpu_fused_launch against a scalar loop, as a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer."""
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "build/test_depth16_native", "-j4"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    r = subprocess.run([os.path.join(csrc, "build", "test_depth16_native")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="3"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "0 failures" in r.stdout
