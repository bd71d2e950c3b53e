"""The unsharp mask without a GPU: the NumPy oracle against an inline
re-statement of the formula, the cpu / omp backends against the oracle, the
batch and mixed-size entry points against the per-image calls, every validation
error and out-of-scope refusal, and the CLI's ``--unsharp``.

Exact bytes only."""
import json
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from conftest import CONV_BIN, PKG

_REF = {}


def _pairs(top):
    return [(1, 0), (16, 0), (255, 0), (24, top // 8), (16, top)]


def _formula(x, b, k, t, top):
    """The definition, restated: python integers, one sample at a time."""
    out = np.empty(x.shape, dtype=x.dtype)
    xf, bf, of = x.reshape(-1), b.reshape(-1), out.reshape(-1)
    for i in range(xf.size):
        xs, bs = int(xf[i]), int(bf[i])
        if abs(xs - bs) < t:
            of[i] = xs
        else:
            of[i] = min(max((xs * (16 + k) - bs * k + 8) >> 4, 0), top)  # python's >> is floor
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_numpy_unsharp_is_the_formula(pconv_mod, dtype):
    top = int(np.iinfo(dtype).max)
    img = np.random.default_rng(12345).integers(0, top + 1, size=(37, 53, 3)).astype(dtype)
    blur = pconv_mod.numpy_convolve(img, 2)
    for k, t in _pairs(top):
        got = pconv_mod.numpy_unsharp(img, 2, k / 16, t)
        assert got.dtype == img.dtype and got.shape == img.shape
        want = _formula(img, blur, k, t, top)
        assert np.array_equal(got, want), (k, t)
        x, b = img.astype(np.int64), blur.astype(np.int64)
        num = x * (16 + k) - b * k + 8
        keep = np.abs(x - b) < t
        if (k, t) == (24, top // 8):
            # the case reaches every branch: clamps at 0 and at max, keeps and changes samples
            counts = (int((~keep & (num < 0)).sum()), int((~keep & ((num >> 4) > top)).sum()), int(keep.sum()),
                      int((got != img).sum()))
            print(np.dtype(dtype).name, "clamped at 0 / clamped at max / kept / changed of", img.size, ":", counts)
            assert all(c > 0 for c in counts), counts
            assert (got[~keep & (num < 0)] == 0).all() and (got[~keep & ((num >> 4) > top)] == top).all()
        if (k, t) == (16, top):
            # |d| < max for every sample of this image: everything is kept
            assert keep.all() and np.array_equal(got, img)
    assert np.array_equal(pconv_mod.numpy_unsharp(img, 0, 1.5, 0), img), "reps = 0 returns the input"


def _image(c, dtype, shape=(37, 53)):
    rng = np.random.default_rng(1009 * c + np.dtype(dtype).itemsize + shape[0])
    full = shape + (c,) if c > 1 else shape
    return rng.integers(0, np.iinfo(dtype).max + 1, size=full).astype(dtype)


def _oracle(pconv_mod, c, dtype, k, t, filt, border):
    """numpy_unsharp of the shared image, computed once per case and never modified."""
    key = (c, np.dtype(dtype).name, k, t, filt, border)
    if key not in _REF:
        _REF[key] = pconv_mod.numpy_unsharp(_image(c, dtype), 3, k / 16, t, filt, border)
        _REF[key].setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("border", ["zero", "replicate"])
@pytest.mark.parametrize("dtype,filt", [(np.uint8, "gaussian"), (np.uint8, "box"), (np.uint16, "gaussian")])
@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_native_backends_equal_the_oracle(pconv_mod, backend, dtype, filt, border):
    import torch

    top = int(np.iinfo(dtype).max)
    for c in (1, 3, 4):
        img = _image(c, dtype)
        for k, t in [(24, top // 8), (255, 0), (1, 1)]:
            want = _oracle(pconv_mod, c, dtype, k, t, filt, border)
            got = pconv_mod.unsharp(img, 3, k / 16, t, filt, backend=backend, border=border)
            assert isinstance(got, np.ndarray) and got.dtype == img.dtype and np.array_equal(got, want), (c, k, t)
            got_t = pconv_mod.unsharp(torch.from_numpy(img), 3, k / 16, t, filt, backend=backend, border=border)
            assert isinstance(got_t, torch.Tensor) and got_t.device.type == "cpu"
            assert got_t.dtype == torch.from_numpy(img).dtype and np.array_equal(got_t.numpy(), want)
    via_numpy = pconv_mod.unsharp(_image(3, dtype), 3, 1.5, top // 8, filt, backend="numpy", border=border)
    assert np.array_equal(via_numpy, _oracle(pconv_mod, 3, dtype, 24, top // 8, filt, border))


@pytest.mark.parametrize("backend", ["numpy", "cpu", "omp"])
def test_reps_zero_returns_the_input(pconv_mod, backend):
    for dtype in (np.uint8, np.uint16):
        img = _image(3, dtype)
        assert np.array_equal(pconv_mod.unsharp(img, 0, 15.9375, 0, backend=backend), img)


@pytest.mark.parametrize("backend", ["numpy", "cpu", "omp"])
def test_batch_and_many_equal_the_per_image_calls(pconv_mod, backend):
    rng = np.random.default_rng(99)
    images = [rng.integers(0, 256, size=sh + (3,), dtype=np.uint8) for sh in [(1, 1), (40, 50), (37, 64)]]
    got = pconv_mod.unsharp_many(images, 3, 1.5, 3, backend=backend, border="replicate")
    assert len(got) == 3
    for g, im in zip(got, images):
        want = pconv_mod.unsharp(im, 3, 1.5, 3, backend=backend, border="replicate")
        assert g.shape == im.shape and np.array_equal(g, want)
        assert np.array_equal(g, pconv_mod.numpy_unsharp(im, 3, 1.5, 3, "gaussian", "replicate"))
    assert pconv_mod.unsharp_many([], 3, 1.5, 3, backend=backend) == []
    for im in images:
        stack = np.stack([im, im[::-1].copy(), im])
        want = np.stack([pconv_mod.unsharp(s, 3, 1.5, 3, backend=backend) for s in stack])
        got = pconv_mod.unsharp_batch(stack, 3, 1.5, 3, backend=backend)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert np.array_equal(pconv_mod.unsharp_batch(list(stack), 3, 1.5, 3, backend=backend), want)
    assert pconv_mod.unsharp_batch(np.stack([images[1]])[:0], 3, backend=backend).shape == (0, 40, 50, 3)
    deep = rng.integers(0, 65536, size=(2, 9, 11, 3)).astype(np.uint16)
    want = np.stack([pconv_mod.numpy_unsharp(im, 2, 2.0, 900) for im in deep])
    assert np.array_equal(pconv_mod.unsharp_batch(deep, 2, 2.0, 900, backend=backend), want)


def test_convolve_file_unsharp(pconv_mod, tmp_path):
    img = _image(3, np.uint8)
    pconv_mod.write_raw(str(tmp_path / "in.raw"), img)
    dst = pconv_mod.convolve_file(str(tmp_path / "in.raw"), 53, 37, 3, "rgb", backend="cpu", unsharp=1.5,
                                  unsharp_threshold=31)
    assert np.array_equal(pconv_mod.read_raw(dst, 53, 37, "rgb"), _oracle(pconv_mod, 3, np.uint8, 24, 31, "gaussian", "zero"))
    with pytest.raises(ValueError, match="unsharp_threshold needs unsharp"):
        pconv_mod.convolve_file(str(tmp_path / "in.raw"), 53, 37, 3, "rgb", backend="cpu", unsharp_threshold=3)
    with pytest.raises(ValueError, match="unsharp: decimate is not supported"):
        pconv_mod.convolve_file(str(tmp_path / "in.raw"), 53, 37, 3, "rgb", backend="cpu", unsharp=1.0, decimate=2)


# ---- validation and refusals ----------------------------------------------------

AMOUNT_ERROR = r"unsharp amount must be a multiple of 1/16 in \[0\.0625, 15\.9375\], got "


@pytest.mark.parametrize("bad", [0, 0.03, 1.01, 16, 15.97, -1.0, "1", None, True, float("nan")])
def test_bad_amount_is_a_value_error(pconv_mod, bad):
    img = _image(3, np.uint8)
    for backend in ("numpy", "cpu", "omp"):
        with pytest.raises(ValueError, match=AMOUNT_ERROR):
            pconv_mod.unsharp(img, 1, bad, backend=backend)
    with pytest.raises(ValueError, match=AMOUNT_ERROR):
        pconv_mod.numpy_unsharp(img, 1, bad)
    with pytest.raises(ValueError, match=AMOUNT_ERROR):
        pconv_mod.unsharp_batch(img[None], 1, bad, backend="cpu")
    with pytest.raises(ValueError, match=AMOUNT_ERROR):
        pconv_mod.unsharp_many([img], 1, bad, backend="omp")


def test_every_multiple_of_a_sixteenth_is_accepted(pconv_mod):
    from pconv.ops.reference import check_unsharp_amount

    assert [check_unsharp_amount(k / 16) for k in range(1, 256)] == list(range(1, 256))
    assert check_unsharp_amount(1) == 16 and check_unsharp_amount(np.float32(0.0625)) == 1


@pytest.mark.parametrize("dtype,bad", [(np.uint8, -1), (np.uint8, 256), (np.uint8, 1.0), (np.uint8, "3"),
                                       (np.uint8, None), (np.uint8, True), (np.uint16, 65536), (np.uint16, -1)])
def test_bad_threshold_is_a_value_error(pconv_mod, dtype, bad):
    img = _image(3, dtype)
    top = int(np.iinfo(dtype).max)
    for backend in ("numpy", "cpu", "omp"):
        with pytest.raises(ValueError, match=rf"unsharp threshold must be an integer in \[0, {top}\], got "):
            pconv_mod.unsharp(img, 1, 1.0, bad, backend=backend)
    with pytest.raises(ValueError, match="unsharp threshold must be an integer"):
        pconv_mod.numpy_unsharp(img, 1, 1.0, bad)
    with pytest.raises(ValueError, match="unsharp threshold must be an integer"):
        pconv_mod.unsharp_batch(img[None], 1, 1.0, bad, backend="cpu")
    with pytest.raises(ValueError, match="unsharp threshold must be an integer"):
        pconv_mod.unsharp_many([img], 1, 1.0, bad, backend="omp")


def test_depth16_keeps_its_rule_and_thresholds_above_255(pconv_mod):
    deep = _image(3, np.uint16)
    for backend in ("numpy", "cpu", "omp"):
        with pytest.raises(ValueError, match="depth 16 .* runs the gaussian filter only"):
            pconv_mod.unsharp(deep, 1, 1.0, 0, "box", backend=backend)
        assert np.array_equal(pconv_mod.unsharp(deep, 2, 1.0, 65535, backend=backend),
                              pconv_mod.numpy_unsharp(deep, 2, 1.0, 65535))


def test_out_of_scope_is_refused_by_name(pconv_mod):
    img = _image(3, np.uint8)
    with pytest.raises(ValueError, match="per-channel amounts are not supported"):
        pconv_mod.unsharp(img, 1, (1.0, 1.0, 2.0), backend="cpu")
    with pytest.raises(ValueError, match="per-channel amounts are not supported"):
        pconv_mod.numpy_unsharp(img, 1, np.array([1.0, 2.0, 1.0]))
    for call in (lambda: pconv_mod.unsharp(img, 1, 1.0, backend="cpu", decimate=2),
                 lambda: pconv_mod.unsharp_batch(img[None], 1, 1.0, backend="cpu", decimate=2),
                 lambda: pconv_mod.unsharp_many([img], 1, 1.0, backend="cpu", decimate=2)):
        with pytest.raises(ValueError, match="unsharp: decimate is not supported"):
            call()
    refused = {
        "pyramid": lambda: pconv_mod.pyramid(img, 2, backend="cpu", unsharp=1.0),
        "Pyramid": lambda: pconv_mod.Pyramid(53, 37, "rgb", 2, unsharp=1.0),
        "FilterPipeline": lambda: pconv_mod.FilterPipeline(["gaussian:1"]).apply(img, backend="cpu", unsharp=1.0),
        "convolve_until_stable": lambda: pconv_mod.convolve_until_stable(img, 4, backend="cpu", unsharp=1.0),
        "convolve_batch_until_stable": lambda: pconv_mod.convolve_batch_until_stable(img[None], 4, backend="cpu",
                                                                                     unsharp=1.0),
        "convolve_many_until_stable": lambda: pconv_mod.convolve_many_until_stable([img], 4, backend="cpu",
                                                                                   unsharp=1.0),
    }
    for name, call in refused.items():
        with pytest.raises(ValueError, match=rf"^{name}: unsharp is not supported"):
            call()


def test_parallel_run_refuses_unsharp(pconv_mod, capsys):
    from pconv.parallel.run import parse

    with pytest.raises(SystemExit):
        parse(["x.raw", "8", "8", "1", "grey", "--unsharp", "1.0"])
    assert "--unsharp is not supported by pconv.parallel.run" in capsys.readouterr().err


def test_native_functions_check_their_arguments(pconv_mod):
    n = pconv_mod.native
    img = _image(3, np.uint8, (13, 21))
    flat, out = img.reshape(-1), np.empty(img.size, np.uint8)
    with pytest.raises(RuntimeError, match="unsharp amount must be a multiple of 1/16"):
        n.cpu_unsharp_convolve(flat, out, 21, 13, "rgb", 1, 0, 0)
    with pytest.raises(RuntimeError, match=r"unsharp threshold must be an integer in \[0, 255\], got 256"):
        n.cpu_unsharp(flat, flat, out, 21, 13, "rgb", 16, 256)
    with pytest.raises(RuntimeError, match="buffer size"):
        n.cpu_unsharp(flat, flat[:-1], out, 21, 13, "rgb", 16, 0)
    with pytest.raises(RuntimeError, match="unsharp amount must be a multiple of 1/16"):
        n.unsharp_k(0.03)
    assert n.unsharp_k(1.5) == 24 and n.UNSHARP_BLOCK_ROWS >= 4 and n.UNSHARP_BLOCK_ROWS % 4 == 0
    blur = pconv_mod.numpy_convolve(img, 2)
    n.cpu_unsharp(flat, blur.reshape(-1), out, 21, 13, "rgb", 24, 3, omp=True)
    assert np.array_equal(out.reshape(img.shape), pconv_mod.numpy_unsharp(img, 2, 1.5, 3))


# ---- CLI ----------------------------------------------------------------------

def _conv(tmp_path, *args):
    return subprocess.run([CONV_BIN, *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _json(r):
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_cli_unsharp(pconv_mod, tmp_path, backend):
    rng = np.random.default_rng(3)
    # three frames from a file, 8 bits, against the NumPy oracle
    frames = rng.integers(0, 256, size=(3, 19, 23, 3), dtype=np.uint8)
    frames.tofile(tmp_path / "three.raw")
    r = _conv(tmp_path, "three.raw", "23", "19", "4", "rgb", "--backend", backend, "--frames", "3", "--unsharp", "1.5",
              "--unsharp-threshold", "3", "--border", "replicate", "--out", "three_out.raw", "--check", "--json",
              "--quiet")
    assert r.returncode == 0, r.stderr
    js = _json(r)
    assert js["mismatches"] == 0 and (js["unsharp"], js["unsharp_threshold"], js["frames"]) == (1.5, 3, 3)
    out = np.fromfile(tmp_path / "three_out.raw", dtype=np.uint8).reshape(3, 19, 23, 3)
    for k in range(3):
        assert np.array_equal(out[k], pconv_mod.numpy_unsharp(frames[k], 4, 1.5, 3, "gaussian", "replicate"))
    # synthetic frames: --check alone
    r = _conv(tmp_path, "s.raw", "40", "29", "5", "rgba", "--backend", backend, "--synthetic", "7", "--frames", "3",
              "--unsharp", "0.0625", "--check", "--json", "--quiet", "--filter", "box")
    assert r.returncode == 0, r.stderr
    js = _json(r)
    assert js["mismatches"] == 0 and (js["unsharp"], js["unsharp_threshold"]) == (0.0625, 0)
    # one frame, 16 bits, a threshold above 255, the default output name
    img = rng.integers(0, 65536, size=(19, 23, 3)).astype(np.uint16)
    img.astype("<u2").tofile(tmp_path / "deep.raw")
    r = _conv(tmp_path, "deep.raw", "23", "19", "4", "rgb", "--backend", backend, "--depth", "16", "--unsharp",
              "15.9375", "--unsharp-threshold", "4000", "--check", "--json", "--quiet")
    assert r.returncode == 0, r.stderr
    js = _json(r)
    assert js["mismatches"] == 0 and (js["unsharp"], js["unsharp_threshold"]) == (15.9375, 4000)
    out = np.fromfile(tmp_path / "blur_deep.raw", dtype="<u2").reshape(19, 23, 3)
    assert np.array_equal(out, pconv_mod.numpy_unsharp(img, 4, 15.9375, 4000))
    # without the option neither key, and the blurred file
    r = _conv(tmp_path, "three.raw", "23", "19", "4", "rgb", "--backend", backend, "--frames", "3", "--out",
              "plain.raw", "--check", "--json", "--quiet")
    assert r.returncode == 0, r.stderr
    assert _json(r)["mismatches"] == 0 and not {"unsharp", "unsharp_threshold"} & set(_json(r))
    plain = np.fromfile(tmp_path / "plain.raw", dtype=np.uint8).reshape(3, 19, 23, 3)
    assert np.array_equal(plain[1], pconv_mod.numpy_convolve(frames[1], 4))


@pytest.mark.parametrize("extra,what", [
    (["--backend", "hip", "--gpus", "2"], "--gpus above 1"),
    (["--server", "/tmp/nowhere.sock"], "--server"),
    (["--bench", "3"], "--bench"),
    (["--backend", "auto"], "--backend auto"),
    (["--converge-every", "4"], "--converge-every"),
    (["--checkpoint-every", "4"], "--checkpoint-every"),
    (["--graph"], "--graph"),
    (["--backend", "cpu", "--decimate", "2"], "--decimate above 1"),
])
def test_cli_usage_errors(tmp_path, extra, what):
    r = _conv(tmp_path, "s.raw", "8", "8", "1", "grey", "--unsharp", "1.0", "--synthetic", "1", *extra)
    assert r.returncode != 0
    assert "--unsharp cannot be combined with " + what in r.stderr, r.stderr
    assert not (tmp_path / "blur_s.raw").exists()


def test_cli_rejects_bad_values_and_documents_the_options(tmp_path):
    base = ("s.raw", "8", "8", "1", "grey", "--synthetic", "1", "--backend", "cpu")
    for bad in ("0", "0.03", "16", "1.01", "-1"):
        r = _conv(tmp_path, *base, "--unsharp", bad)
        assert r.returncode != 0 and "unsharp amount must be a multiple of 1/16 in [0.0625, 15.9375], got" in r.stderr
    for bad in ("one", "1.5x", ""):
        r = _conv(tmp_path, *base, "--unsharp", bad)
        assert r.returncode != 0 and "invalid --unsharp" in r.stderr, r.stderr
    r = _conv(tmp_path, *base, "--unsharp-threshold", "3")
    assert r.returncode != 0 and "--unsharp-threshold needs --unsharp" in r.stderr
    r = _conv(tmp_path, *base, "--unsharp", "1.0", "--unsharp-threshold", "256")
    assert r.returncode != 0 and "unsharp threshold must be an integer in [0, 255], got 256" in r.stderr
    r = _conv(tmp_path, *base, "--unsharp", "1.0", "--unsharp-threshold", "-1")
    assert r.returncode != 0 and "invalid --unsharp-threshold" in r.stderr
    r = _conv(tmp_path, *base, "--unsharp", "1.0", "--depth", "16", "--unsharp-threshold", "65535", "--quiet")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "blur_s.raw").stat().st_size == 8 * 8 * 2
    r = _conv(tmp_path, "--help")
    text = r.stdout + r.stderr
    assert "--unsharp A" in text and "--unsharp-threshold T" in text and "multiple of 1/16" in text


def test_a_served_job_is_refused(pconv_mod, tmp_path):
    from pconv.utils.service import ServiceClient, ServiceError

    sock = "/tmp/pconv-unsharp-%d.sock" % os.getpid()
    p = subprocess.Popen([CONV_BIN, "--serve", sock, "--device", "-1", "--idle-timeout", "300"],
                         stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(600):
            if os.path.exists(sock):
                break
            assert p.poll() is None, p.stderr.read()
            time.sleep(0.05)
        reply = ServiceClient(sock).request("conv", "s.raw", "8", "8", "1", "grey", "--synthetic", "1", "--backend",
                                            "cpu", "--unsharp", "1.0", "--out", str(tmp_path / "o.raw"))
        assert "--unsharp cannot run as a served job" in reply.get("error", ""), reply
        assert not (tmp_path / "o.raw").exists()
        # the Python client (and a ServicePool's workers, which call it) raise the same refusal
        with pytest.raises(ServiceError, match="--unsharp cannot run as a served job"):
            ServiceClient(sock).run("s.raw", 8, 8, 1, "grey", out=str(tmp_path / "o.raw"), synthetic=1,
                                    backend="cpu", unsharp=1.0)
        ServiceClient(sock).shutdown()
    finally:
        if p.poll() is None:
            try:
                ServiceClient(sock).shutdown()
            except Exception:
                p.kill()
        p.wait(timeout=60)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_unsharp_native_runner_asan_ubsan():
    """tests/cpp/test_unsharp_native.cpp: cpu_unsharp and cpu_unsharp_convolve
    against a scalar loop into exact-size heap buffers, as a stand-alone program
    under AddressSanitizer + UndefinedBehaviorSanitizer."""
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "build/test_unsharp_native", "-j4"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    r = subprocess.run([os.path.join(csrc, "build", "test_unsharp_native")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="3"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
