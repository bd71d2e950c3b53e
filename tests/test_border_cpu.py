"""Replicate border (`border="replicate"`) on the CPU paths: the NumPy oracle
against a direct clamp-index evaluation, the C++ oracle (serial and OpenMP)
against the NumPy one, band frames of a fused launch, the distributed CPU
emulator, the CLI and the resident service.

Semantics, per channel and repetition:
    out[y][x] = trunc(sum_{k,l} w[k][l] * in[clamp(y+k-1, 0, H-1)][clamp(x+l-1, 0, W-1)])
with the project's float32 mul-then-add in row-major tap order (the integer
formula for int_exact filters); `zero` stays the default and the reference's
contract."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import CONV_BIN

CH = {"grey": 1, "rgb": 3, "rgba": 4}
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py
INT_TAPS = ([1, 0, 3, 2, 4, 0, 1, 3, 2], 16)   # int_exact (non-negative taps, power-of-two divisor), not the gaussian
SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (17, 16), (31, 100)]


def _filter(pconv_mod, name):
    if name == "neg":
        return pconv_mod.get_filter(NEG_TAPS)
    if name == "int":
        f = pconv_mod.get_filter(INT_TAPS)
        assert f.int_exact and not f.to_native().binomial121
        return f
    return pconv_mod.get_filter(name)


def _image(rng, h, w, channels):
    c = CH[channels]
    return rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


def _clamp_step(img, f):
    """One repetition, pixel by pixel, straight from the formula."""
    x = img if img.ndim == 3 else img[:, :, None]
    h, w, c = x.shape
    out = np.empty_like(x)
    w32 = np.asarray(f.weights32, np.float32).reshape(3, 3)
    for y in range(h):
        for xx in range(w):
            for ch in range(c):
                if f.int_exact:
                    acc = 0
                    for k in range(3):
                        for l in range(3):
                            acc += f.taps[3 * k + l] * int(x[min(max(y + k - 1, 0), h - 1), min(max(xx + l - 1, 0), w - 1), ch])
                    out[y, xx, ch] = min(acc >> f.shift, 255)
                else:
                    acc = np.float32(0.0)
                    for k in range(3):
                        for l in range(3):
                            p = np.float32(x[min(max(y + k - 1, 0), h - 1), min(max(xx + l - 1, 0), w - 1), ch])
                            acc = np.float32(acc + np.float32(p * w32[k, l]))
                    out[y, xx, ch] = 0 if not acc > 0 else min(int(np.trunc(acc)), 255)
    return out.reshape(img.shape)


@pytest.mark.parametrize("filt", ["gaussian", "box", "edge", "neg", "int"])
def test_numpy_oracle_equals_clamp_index_evaluation(pconv_mod, rng, filt):
    f = _filter(pconv_mod, filt)
    for channels in ("grey", "rgb"):
        for (h, w) in [(1, 1), (1, 4), (3, 1), (2, 2), (4, 5)]:
            img = _image(rng, h, w, channels)
            want = img
            for _ in range(3):
                want = _clamp_step(want, f)
            assert np.array_equal(pconv_mod.numpy_convolve(img, 3, f, border="replicate"), want), (channels, h, w)


def test_unknown_border_is_rejected(pconv_mod):
    img = np.zeros((3, 3), np.uint8)
    with pytest.raises(ValueError, match="border"):
        pconv_mod.numpy_convolve(img, 1, "gaussian", border="wrap")
    with pytest.raises(ValueError, match="border"):
        pconv_mod.convolve(img, 1, backend="cpu", border="wrap")
    with pytest.raises(RuntimeError, match="unknown border"):
        pconv_mod.native.cpu_convolve(img.reshape(-1), img.copy().reshape(-1), 3, 3, "grey", 1, "gaussian", False, 0,
                                      border="wrap")


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("filt", ["gaussian", "box", "edge", "neg", "int"])
def test_cpu_convolve_equals_numpy_oracle(pconv_mod, rng, channels, filt):
    f = _filter(pconv_mod, filt)
    for (h, w) in SIZES:
        img = _image(rng, h, w, channels)
        for reps in (1, 2, 7):
            ref = pconv_mod.numpy_convolve(img, reps, f, border="replicate")
            for backend in ("cpu", "omp"):
                src = img.copy()
                got = pconv_mod.convolve(src, reps, f, backend=backend, border="replicate")
                assert np.array_equal(got, ref), (backend, h, w, reps)
                assert np.array_equal(src, img), "the input image was modified"


def test_default_border_is_zero_and_positional_calls_still_work(pconv_mod, rng):
    n = pconv_mod.native
    img = _image(rng, 9, 11, "rgb")
    ref = pconv_mod.numpy_convolve(img, 3)
    assert np.array_equal(pconv_mod.numpy_convolve(img, 3, "gaussian", "zero"), ref)
    out = np.empty_like(img)
    n.cpu_convolve(img.reshape(-1), out.reshape(-1), 11, 9, "rgb", 3, "gaussian", False, 0)  # as before this option
    assert np.array_equal(out, ref)
    assert np.array_equal(pconv_mod.convolve(img, 3, backend="cpu", border="zero"), ref)
    assert list(n.border_names()) == ["zero", "replicate"]


def test_constant_image_stays_constant_only_with_replicate(pconv_mod):
    """The reason for the option: 40 gaussian repetitions leave a constant
    image constant under replicate, and darken its frame under zero."""
    img = np.full((24, 31, 3), 200, np.uint8)
    for backend in ("numpy", "cpu", "omp"):
        rep = pconv_mod.convolve(img, 40, "gaussian", backend=backend, border="replicate")
        assert (rep == 200).all(), backend
        zero = pconv_mod.convolve(img, 40, "gaussian", backend=backend)
        assert zero[0, 0, 0] < 100 and (zero != 200).any(), backend
    pipe = pconv_mod.FilterPipeline.from_spec("gaussian:5,gaussian:3")
    assert (pipe.apply(img, backend="cpu", border="replicate") == 200).all()
    assert (pipe.reference(img, border="replicate") == 200).all()
    assert (pipe.apply(img, backend="cpu") != 200).any()


def _band_frame(native, img, y0, rows, halo, fill):
    """Frame (pitched, pads zero) of band rows [y0, y0 + rows) of `img` with its
    ghost rows: image rows where they exist, `fill` outside the image."""
    h = img.shape[0]
    rb = img.size // h
    lay = native.frame_layout(rb, rows, halo)
    fr = np.zeros((rows + 2 * halo, lay["pitch"]), np.uint8)
    flat = img.reshape(h, rb)
    for r in range(-halo, rows + halo):
        g = y0 + r
        fr[halo + r, 16:16 + rb] = flat[g] if 0 <= g < h else fill
    return lay, fr


@pytest.mark.parametrize("filt", ["gaussian", "edge", "int"])
@pytest.mark.parametrize("steps", [1, 3])
def test_fused_launch_on_band_frames(pconv_mod, rng, filt, steps):
    n = pconv_mod.native
    f = _filter(pconv_mod, filt)
    H, W, halo = 20, 7, 4
    img = _image(rng, H, W, "rgb")
    ref = pconv_mod.numpy_convolve(img, steps, f, border="replicate").reshape(H, -1)
    # (y0, rows): only the bottom is an image edge / ghost rows above the image hold 0xEE
    for y0, rows in ((12, 8), (0, 9)):
        lay, fr = _band_frame(n, img, y0, rows, halo, 0xEE)
        src = fr.copy()
        dst = np.zeros_like(fr)
        n.cpu_fused_launch(f.to_native(), "rgb", 3 * W, rows, halo, src.reshape(-1), dst.reshape(-1), 0, rows, steps,
                           y0, H, False, border="replicate")
        assert np.array_equal(src, fr), "the source frame was modified"
        assert np.array_equal(dst[halo:halo + rows, 16:16 + 3 * W], ref[y0:y0 + rows]), (y0, rows)
        assert (dst[:halo] == 0).all() and (dst[halo + rows:] == 0).all()
        assert (dst[:, :16] == 0).all() and (dst[:, 16 + 3 * W:] == 0).all()


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("height", [8, 50])
def test_cpu_cluster_emulator_equals_oracle(pconv_mod, rng, world, height):
    from pconv.parallel.cpu_dist import local_cpu_cluster_convolve

    img = _image(rng, height, 13, "rgb")
    ref = pconv_mod.numpy_convolve(img, 9, "gaussian", border="replicate")
    for halo in (1, 4):
        for fuse in (1, 3, 8):
            got = local_cpu_cluster_convolve(img, 9, world, halo=halo, fuse=fuse, border="replicate")
            assert np.array_equal(got, ref), (world, height, halo, fuse)
    box = pconv_mod.numpy_convolve(img, 4, "box", border="replicate")
    assert np.array_equal(local_cpu_cluster_convolve(img, 4, world, "box", halo=2, fuse=2, preload_halo=True,
                                                     border="replicate"), box)


def _run(args, cwd):
    return subprocess.run([CONV_BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_cli_replicate_output_equals_oracle(pconv_mod, tmp_path, backend):
    r = _run(["s.raw", "37", "29", "6", "rgb", "--synthetic", "1", "--backend", backend, "--border", "replicate",
              "--check", "--json", "--quiet"], tmp_path)
    assert r.returncode == 0, r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["border"] == "replicate" and meta["mismatches"] == 0
    out = pconv_mod.read_raw(str(tmp_path / "blur_s.raw"), 37, 29, "rgb")
    img = pconv_mod.synthetic_image(37, 29, "rgb", seed=1)
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, 6, border="replicate"))
    assert not np.array_equal(out, pconv_mod.numpy_convolve(img, 6))
    # the default echoes "zero" and is today's result
    r = _run(["s.raw", "37", "29", "6", "rgb", "--synthetic", "1", "--backend", backend, "--json", "--quiet"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["border"] == "zero"
    assert np.array_equal(pconv_mod.read_raw(str(tmp_path / "blur_s.raw"), 37, 29, "rgb"),
                          pconv_mod.numpy_convolve(img, 6))


def test_cli_unknown_border_is_a_usage_error(tmp_path):
    r = _run(["s.raw", "8", "8", "1", "grey", "--synthetic", "1", "--backend", "cpu", "--border", "bogus"], tmp_path)
    assert r.returncode == 1 and "invalid --border 'bogus'" in r.stderr and "Error Input!" in r.stderr
    assert not os.path.exists(tmp_path / "blur_s.raw")
    r = _run(["s.raw", "8", "8", "1", "grey", "--border"], tmp_path)
    assert r.returncode == 1 and "missing value for --border" in r.stderr
    assert "--border {zero,replicate}" in _run(["--help"], tmp_path).stdout


def test_cli_checkpoints_and_auto_backend_under_replicate(pconv_mod, tmp_path):
    img = pconv_mod.synthetic_image(21, 18, "grey", seed=3)
    r = _run(["s.raw", "21", "18", "5", "grey", "--synthetic", "3", "--backend", "cpu", "--border", "replicate",
              "--checkpoint-every", "2", "--quiet"], tmp_path)
    assert r.returncode == 0, r.stderr
    for k in (2, 4):
        got = pconv_mod.read_raw(str(tmp_path / f"blur_s.raw.rep{k}"), 21, 18, "grey")
        assert np.array_equal(got, pconv_mod.numpy_convolve(img, k, border="replicate")), k
    # a job this small is priced on the CPU and stays there (no GPU is touched)
    r = _run(["s.raw", "21", "18", "5", "grey", "--synthetic", "3", "--backend", "auto", "--border", "replicate",
              "--check", "--quiet"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pconv_mod.read_raw(str(tmp_path / "blur_s.raw"), 21, 18, "grey"),
                          pconv_mod.numpy_convolve(img, 5, border="replicate"))


def test_service_keeps_borders_apart(pconv_mod, tmp_path, rng):
    """Two jobs of one geometry that differ only in the border, on one resident
    (`--device -1`) server, each return their own correct bytes, in either order."""
    from pconv.utils.service import ServiceClient

    sock = "/tmp/pconv-border-%d.sock" % os.getpid()
    p = subprocess.Popen([CONV_BIN, "--serve", sock, "--device", "-1", "--idle-timeout", "300"],
                         stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(600):
            if os.path.exists(sock):
                break
            assert p.poll() is None, p.stderr.read()
            time.sleep(0.05)
        img = rng.integers(0, 256, size=(23, 19, 3), dtype=np.uint8)
        pconv_mod.write_raw(str(tmp_path / "in.raw"), img)
        c = ServiceClient(sock)
        for border in ("replicate", "zero", "replicate"):
            out = str(tmp_path / f"out_{border}.raw")
            meta = c.run(str(tmp_path / "in.raw"), 19, 23, 5, "rgb", out=out, backend="omp", border=border, check=True)
            assert meta["border"] == border and meta["mismatches"] == 0
            assert np.array_equal(pconv_mod.read_raw(out, 19, 23, "rgb"),
                                  pconv_mod.numpy_convolve(img, 5, border=border)), border
        assert not np.array_equal(pconv_mod.read_raw(str(tmp_path / "out_zero.raw"), 19, 23, "rgb"),
                                  pconv_mod.read_raw(str(tmp_path / "out_replicate.raw"), 19, 23, "rgb"))
        c.shutdown()
    finally:
        if p.poll() is None:
            try:
                ServiceClient(sock).shutdown()
            except Exception:
                p.kill()
        p.wait(timeout=60)
