"""Decimated results and pyramids without a GPU: the ``decimate`` keyword on the
numpy / cpu / omp backends against ``numpy_convolve(...)[::s, ::s]``, the batch
and mixed-size entry points against the per-image calls, the pyramid's
definition and limits, and the CLI's ``--decimate``.

Exact bytes only."""
import json
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from conftest import CONV_BIN, PKG

BACKENDS = ["numpy", "cpu", "omp"]
FACTORS = [1, 2, 3, 7, 64]
SHAPES = [(1, 1), (1, 9), (9, 1), (13, 21), (64, 64)]
CHANNELS = [1, 3, 4]

_IMG = {}
_REF = {}


def _image(shape, c, dtype):
    key = (shape, c, np.dtype(dtype).name)
    if key not in _IMG:
        rng = np.random.default_rng(1009 * shape[0] + 31 * shape[1] + c + np.dtype(dtype).itemsize)
        full = shape + (c,) if c > 1 else shape
        _IMG[key] = rng.integers(0, np.iinfo(dtype).max + 1, size=full).astype(dtype)
    return _IMG[key]


def _oracle(pconv_mod, shape, c, dtype, reps, filt, border):
    """numpy_convolve of the shared image, computed once per case and never modified."""
    key = (shape, c, np.dtype(dtype).name, reps, filt, border)
    if key not in _REF:
        _REF[key] = pconv_mod.numpy_convolve(_image(shape, c, dtype), reps, filt, border)
        _REF[key].setflags(write=False)
    return _REF[key]


@pytest.mark.parametrize("border", ["zero", "replicate"])
@pytest.mark.parametrize("dtype,filt", [(np.uint8, "gaussian"), (np.uint8, "box"), (np.uint16, "gaussian")])
@pytest.mark.parametrize("backend", BACKENDS)
def test_convolve_decimate_equals_sliced_oracle(pconv_mod, backend, dtype, filt, border):
    for shape in SHAPES:
        for c in CHANNELS:
            img = _image(shape, c, dtype)
            full = _oracle(pconv_mod, shape, c, dtype, 3, filt, border)
            for s in FACTORS:
                got = pconv_mod.convolve(img, 3, filt, backend=backend, border=border, decimate=s)
                want = full[::s, ::s]
                assert isinstance(got, np.ndarray) and got.dtype == img.dtype
                assert got.shape == want.shape == (-(-shape[0] // s), -(-shape[1] // s)) + img.shape[2:]
                assert np.array_equal(got, want), (backend, shape, c, s)
                assert np.array_equal(pconv_mod.numpy_decimate(full, s), want)


def test_decimate_one_is_the_plain_call_and_tensors_keep_their_container(pconv_mod):
    import torch

    img = _image((13, 21), 3, np.uint8)
    for backend in BACKENDS:
        assert np.array_equal(pconv_mod.convolve(img, 4, backend=backend, decimate=1),
                              pconv_mod.convolve(img, 4, backend=backend))
        t = pconv_mod.convolve(torch.from_numpy(img), 4, backend=backend, decimate=3)
        assert isinstance(t, torch.Tensor) and t.device.type == "cpu"
        assert np.array_equal(t.numpy(), _oracle(pconv_mod, (13, 21), 3, np.uint8, 4, "gaussian", "zero")[::3, ::3])


@pytest.mark.parametrize("backend", BACKENDS)
def test_batch_and_many_equal_the_per_image_calls(pconv_mod, backend):
    rng = np.random.default_rng(99)
    stack = rng.integers(0, 256, size=(3, 13, 21, 3), dtype=np.uint8)
    for s in (2, 7):
        want = np.stack([pconv_mod.convolve(im, 3, backend=backend, decimate=s) for im in stack])
        got = pconv_mod.convolve_batch(stack, 3, backend=backend, decimate=s)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert np.array_equal(want, np.stack([pconv_mod.numpy_convolve(im, 3)[::s, ::s] for im in stack]))
    empty = pconv_mod.convolve_batch(stack[:0], 3, backend=backend, decimate=2)
    assert empty.shape == (0, 7, 11, 3)
    images = [rng.integers(0, 256, size=sh, dtype=np.uint8) for sh in [(13, 21, 3), (1, 1, 3), (9, 4, 3), (30, 2, 3)]]
    for s in (2, 3):
        got = pconv_mod.convolve_many(images, 3, backend=backend, border="replicate", decimate=s)
        for g, im in zip(got, images):
            want = pconv_mod.convolve(im, 3, backend=backend, border="replicate", decimate=s)
            assert g.shape == want.shape and np.array_equal(g, want)
            assert np.array_equal(g, pconv_mod.numpy_convolve(im, 3, "gaussian", "replicate")[::s, ::s])


def test_filter_pipeline_decimates_after_the_last_stage(pconv_mod):
    img = _image((13, 21), 3, np.uint8)
    pipe = pconv_mod.FilterPipeline.from_spec("gaussian:3,box:2")
    full = pipe.reference(img)
    assert np.array_equal(pipe.reference(img, decimate=3), full[::3, ::3])
    for backend in BACKENDS:
        assert np.array_equal(pipe.apply(img, backend=backend, decimate=3), full[::3, ::3])
        assert np.array_equal(pipe.apply(img, backend=backend), full)


def test_convolve_file_decimates(pconv_mod, tmp_path):
    img = _image((13, 21), 3, np.uint8)
    pconv_mod.write_raw(str(tmp_path / "in.raw"), img)
    dst = pconv_mod.convolve_file(str(tmp_path / "in.raw"), 21, 13, 3, "rgb", backend="cpu", decimate=2)
    want = _oracle(pconv_mod, (13, 21), 3, np.uint8, 3, "gaussian", "zero")[::2, ::2]
    assert np.array_equal(pconv_mod.read_raw(dst, 11, 7, "rgb"), want)


@pytest.mark.parametrize("backend", BACKENDS)
def test_pyramid_definition_and_limits(pconv_mod, backend):
    for shape, c, most in [((13, 21), 3, 6), ((64, 64), 1, 7), ((1, 9), 1, 5), ((1, 1), 4, 1)]:
        img = _image(shape, c, np.uint8)
        for reps in (2, 0):
            pyr = pconv_mod.pyramid(img, most, reps, backend=backend, border="replicate")
            assert len(pyr) == most and np.array_equal(pyr[0], img)
            assert pyr[-1].shape[:2] == (1, 1)
            for k in range(most - 1):
                nxt = pconv_mod.convolve(pyr[k], reps, backend=backend, border="replicate", decimate=2)
                assert pyr[k + 1].shape == nxt.shape and np.array_equal(pyr[k + 1], nxt)
                assert np.array_equal(nxt, pconv_mod.numpy_convolve(pyr[k], reps, "gaussian", "replicate")[::2, ::2])
        assert len(pconv_mod.pyramid(img, 1, backend=backend)) == 1
        with pytest.raises(ValueError, match="levels"):
            pconv_mod.pyramid(img, most + 1, backend=backend)
        for bad in (0, -1, 1.5, "2"):
            with pytest.raises(ValueError, match="levels"):
                pconv_mod.pyramid(img, bad, backend=backend)
    assert pconv_mod.ops.pyramid_sizes(21, 13) == [(21, 13), (11, 7), (6, 4), (3, 2), (2, 1), (1, 1)]


@pytest.mark.parametrize("bad", [0, -2, 65, 2.0, "2", None, True])
def test_bad_factor_is_a_value_error(pconv_mod, bad):
    img = _image((13, 21), 3, np.uint8)
    with pytest.raises(ValueError, match="decimate"):
        pconv_mod.convolve(img, 1, backend="cpu", decimate=bad)
    with pytest.raises(ValueError, match="decimate"):
        pconv_mod.convolve_batch(img[None], 1, backend="numpy", decimate=bad)
    with pytest.raises(ValueError, match="decimate"):
        pconv_mod.convolve_many([img], 1, backend="omp", decimate=bad)
    with pytest.raises(ValueError, match="decimate"):
        pconv_mod.numpy_decimate(img, bad)
    with pytest.raises(ValueError, match="decimate"):
        pconv_mod.FilterPipeline(["gaussian:1"]).apply(img, backend="cpu", decimate=bad)


def test_native_cpu_convolve_checks_factor_and_buffer(pconv_mod):
    img = _image((13, 21), 3, np.uint8)
    n = pconv_mod.native
    with pytest.raises(RuntimeError, match="decimate 65 is outside"):
        n.cpu_convolve(img.reshape(-1), np.empty(img.size, np.uint8), 21, 13, "rgb", 1, decimate=65)
    with pytest.raises(RuntimeError, match="buffer size"):
        n.cpu_convolve(img.reshape(-1), np.empty(img.size, np.uint8), 21, 13, "rgb", 1, decimate=2)
    assert n.MAX_DECIMATE == 64


# ---- CLI ----------------------------------------------------------------------

def _conv(tmp_path, *args):
    return subprocess.run([CONV_BIN, *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _json(r):
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_cli_decimate(pconv_mod, tmp_path, backend):
    rng = np.random.default_rng(3)
    # two frames, 8 bits
    frames = rng.integers(0, 256, size=(2, 19, 23, 3), dtype=np.uint8)
    frames.tofile(tmp_path / "two.raw")
    r = _conv(tmp_path, "two.raw", "23", "19", "4", "rgb", "--backend", backend, "--frames", "2", "--decimate", "3",
              "--border", "replicate", "--out", "two_out.raw", "--check", "--json", "--quiet")
    assert r.returncode == 0, r.stderr
    js = _json(r)
    assert js["mismatches"] == 0
    assert (js["decimate"], js["out_width"], js["out_height"], js["frames"]) == (3, 8, 7, 2)
    assert os.path.getsize(tmp_path / "two_out.raw") == 2 * 7 * 8 * 3
    out = np.fromfile(tmp_path / "two_out.raw", dtype=np.uint8).reshape(2, 7, 8, 3)
    for k in range(2):
        assert np.array_equal(out[k], pconv_mod.numpy_convolve(frames[k], 4, "gaussian", "replicate")[::3, ::3])
    # one frame, 16 bits, the default output name
    img = rng.integers(0, 65536, size=(19, 23, 3)).astype(np.uint16)
    img.astype("<u2").tofile(tmp_path / "deep.raw")
    r = _conv(tmp_path, "deep.raw", "23", "19", "4", "rgb", "--backend", backend, "--depth", "16", "--decimate", "3",
              "--check", "--json", "--quiet")
    assert r.returncode == 0, r.stderr
    js = _json(r)
    assert js["mismatches"] == 0 and (js["decimate"], js["out_width"], js["out_height"]) == (3, 8, 7)
    assert os.path.getsize(tmp_path / "blur_deep.raw") == 7 * 8 * 3 * 2
    out = np.fromfile(tmp_path / "blur_deep.raw", dtype="<u2").reshape(7, 8, 3)
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, 4)[::3, ::3])
    # without the flag (and with --decimate 1) none of the three keys, and the full-size file
    for extra in ([], ["--decimate", "1"]):
        r = _conv(tmp_path, "two.raw", "23", "19", "4", "rgb", "--backend", backend, "--frames", "2", "--out",
                  "plain.raw", "--check", "--json", "--quiet", *extra)
        assert r.returncode == 0, r.stderr
        js = _json(r)
        assert js["mismatches"] == 0 and not {"decimate", "out_width", "out_height"} & set(js)
        assert os.path.getsize(tmp_path / "plain.raw") == frames.size


@pytest.mark.parametrize("extra,what", [
    (["--backend", "hip", "--gpus", "2"], "--gpus above 1"),
    (["--server", "/tmp/nowhere.sock"], "--server"),
    (["--bench", "3"], "--bench"),
    (["--backend", "auto"], "--backend auto"),
    (["--converge-every", "4"], "--converge-every"),
    (["--checkpoint-every", "4"], "--checkpoint-every"),
])
def test_cli_usage_errors(tmp_path, extra, what):
    r = _conv(tmp_path, "s.raw", "8", "8", "1", "grey", "--decimate", "2", "--synthetic", "1", *extra)
    assert r.returncode != 0
    assert "--decimate above 1 cannot be combined with " + what in r.stderr, r.stderr
    assert not (tmp_path / "blur_s.raw").exists()


def test_cli_rejects_other_factors_and_documents_the_flag(tmp_path):
    for bad in ("0", "65", "two"):
        r = _conv(tmp_path, "s.raw", "8", "8", "1", "grey", "--decimate", bad, "--synthetic", "1", "--backend", "cpu")
        assert r.returncode != 0 and "invalid --decimate" in r.stderr
    r = _conv(tmp_path, "--help")
    assert "--decimate S" in r.stdout + r.stderr


def test_a_served_job_is_refused(pconv_mod, tmp_path):
    from pconv.utils.service import ServiceClient

    sock = "/tmp/pconv-decimate-%d.sock" % os.getpid()
    p = subprocess.Popen([CONV_BIN, "--serve", sock, "--device", "-1", "--idle-timeout", "300"],
                         stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(600):
            if os.path.exists(sock):
                break
            assert p.poll() is None, p.stderr.read()
            time.sleep(0.05)
        reply = ServiceClient(sock).request("conv", "s.raw", "8", "8", "1", "grey", "--synthetic", "1", "--backend",
                                            "cpu", "--decimate", "2", "--out", str(tmp_path / "o.raw"))
        assert "--decimate above 1 cannot run as a served job" in reply.get("error", ""), reply
        assert not (tmp_path / "o.raw").exists()
        ServiceClient(sock).shutdown()
    finally:
        if p.poll() is None:
            try:
                ServiceClient(sock).shutdown()
            except Exception:
                p.kill()
        p.wait(timeout=60)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_decimate_native_runner_asan_ubsan():
    """tests/cpp/test_decimate_native.cpp: copy_out_decimated and cpu_convolve's
    decimate against a scalar loop into exact-size heap buffers, as a
    stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "build/test_decimate_native", "-j4"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    r = subprocess.run([os.path.join(csrc, "build", "test_decimate_native")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="3"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
