"""Image batches without a GPU: ``convolve_batch`` on the CPU backends, the
``--frames`` flag of the CLI on ``cpu`` / ``omp``, and the latency model's
batch argument.

Every batch result is compared with the stacked single-image NumPy oracle:
a batch is N independent images, nothing else."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import CONV_BIN

NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py
H, W = 7, 9
BACKENDS = ["numpy", "cpu", "omp"]
BORDERS = ["zero", "replicate"]
REPS = 3

_REF = {}  # (shape, filter key, border) -> stacked oracle, computed once and shared by the backends


def _stack(shape):
    rng = np.random.default_rng(sum(s * 31 ** i for i, s in enumerate(shape)))
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def _filters(pconv_mod):
    return [(name, name) for name in pconv_mod.list_filters()] + [("neg", NEG_TAPS)]


def _oracle(pconv_mod, stack, fkey, filt, border):
    key = (stack.shape, fkey, border)
    if key not in _REF:
        outs = [pconv_mod.numpy_convolve(stack[i], REPS, filt, border=border) for i in range(stack.shape[0])]
        _REF[key] = np.stack(outs) if outs else np.empty(stack.shape, np.uint8)
    return _REF[key]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_convolve_batch_equals_stacked_single_images(pconv_mod, backend, border):
    for n in (0, 1, 5):
        for tail in ((), (3,), (4,)):
            stack = _stack((n, H, W) + tail)
            for fkey, filt in _filters(pconv_mod):
                ref = _oracle(pconv_mod, stack, fkey, filt, border)
                case = (backend, border, n, tail, fkey)
                got = pconv_mod.convolve_batch(stack, REPS, filt, backend=backend, border=border)
                assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == stack.shape, case
                assert np.array_equal(got, ref), case
                # a list of arrays is stacked (an empty list has no geometry: an error, below)
                if n:
                    got = pconv_mod.convolve_batch([stack[i] for i in range(n)], REPS, filt, backend=backend,
                                                   border=border)
                    assert isinstance(got, np.ndarray) and np.array_equal(got, ref), case
                # a CPU tensor comes back as a CPU tensor
                got = pconv_mod.convolve_batch(torch.from_numpy(stack), REPS, filt, backend=backend, border=border)
                assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and not got.is_cuda, case
                assert tuple(got.shape) == stack.shape and np.array_equal(got.numpy(), ref), case


def test_convolve_batch_batch_size_is_ignored_off_the_gpu(pconv_mod):
    stack = _stack((5, H, W, 3))
    ref = _oracle(pconv_mod, stack, "gaussian", "gaussian", "zero")
    assert np.array_equal(pconv_mod.convolve_batch(stack, REPS, backend="omp", batch_size=2), ref)


def test_convolve_batch_rejections(pconv_mod):
    with pytest.raises(TypeError, match="uint8"):
        pconv_mod.convolve_batch(torch.zeros((2, H, W), dtype=torch.float32), backend="numpy")
    with pytest.raises(TypeError, match="uint8"):
        pconv_mod.convolve_batch(np.zeros((2, H, W), np.int16), backend="numpy")
    with pytest.raises(ValueError, match="one shape"):
        pconv_mod.convolve_batch([np.zeros((H, W), np.uint8), np.zeros((H, W + 1), np.uint8)], backend="numpy")
    with pytest.raises(ValueError, match="batch shape"):
        pconv_mod.convolve_batch(np.zeros((H, W), np.uint8), backend="numpy")
    with pytest.raises(ValueError, match="batch_size"):
        pconv_mod.convolve_batch(np.zeros((2, H, W), np.uint8), backend="numpy", batch_size=0)
    with pytest.raises(ValueError, match="reps"):
        pconv_mod.convolve_batch(np.zeros((2, H, W), np.uint8), reps=-1, backend="numpy")
    with pytest.raises(ValueError):
        pconv_mod.convolve_batch([], backend="numpy")
    # convolve itself still takes one image
    with pytest.raises(ValueError, match="unsupported image shape"):
        pconv_mod.convolve(np.zeros((2, H, W, 3), np.uint8), backend="numpy")


# ---- CLI ---------------------------------------------------------------

CW, CH_, CREPS = 40, 30, 4


def _run(args, cwd):
    return subprocess.run([CONV_BIN] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("backend", ["omp", "cpu"])
def test_cli_frames_synthetic(pconv_mod, tmp_path, backend):
    r = _run(["s.raw", CW, CH_, CREPS, "rgb", "--backend", backend, "--synthetic", 9, "--frames", 3, "--check",
              "--json", "--quiet", "--out", "out.raw"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "check: 0 mismatching bytes" in r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["frames"] == 3 and js["mismatches"] == 0 and js["reps"] == CREPS
    # Mpix/s counts all frames
    assert js["loop_mpix_per_s"] == pytest.approx(CW * CH_ * 3 * CREPS / js["loop_s"] / 1e6, rel=1e-3)
    out = np.fromfile(tmp_path / "out.raw", dtype=np.uint8)
    assert out.size == 3 * CW * CH_ * 3
    out = out.reshape(3, CH_, CW, 3)
    for k in range(3):  # frame k comes from seed 9 + k
        src = pconv_mod.synthetic_image(CW, CH_, "rgb", seed=9 + k)
        assert np.array_equal(out[k], pconv_mod.numpy_convolve(src, CREPS, "gaussian")), k


@pytest.mark.parametrize("backend", ["omp", "cpu"])
def test_cli_frames_from_file(pconv_mod, tmp_path, backend):
    stack = _stack((3, CH_, CW, 3))
    stack.tofile(tmp_path / "in.raw")
    r = _run(["in.raw", CW, CH_, 2, "rgb", "--backend", backend, "--frames", 3, "--filter", "box", "--border",
              "replicate", "--quiet"], tmp_path)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "blur_in.raw", dtype=np.uint8).reshape(stack.shape)
    for k in range(3):
        assert np.array_equal(out[k], pconv_mod.numpy_convolve(stack[k], 2, "box", border="replicate")), k
    # one byte short: an error, like every input size
    stack.reshape(-1)[:-1].tofile(tmp_path / "short.raw")
    r = _run(["short.raw", CW, CH_, 2, "rgb", "--backend", backend, "--frames", 3], tmp_path)
    assert r.returncode == 1 and "needs" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "blur_short.raw")


def test_cli_frames_usage_errors(tmp_path):
    base = ["s.raw", CW, CH_, CREPS, "rgb", "--synthetic", 1]
    for bad in ("0", "x", "-2"):
        r = _run(base + ["--backend", "omp", "--frames", bad], tmp_path)
        assert r.returncode == 1 and "--frames" in r.stderr and "Error Input!" in r.stderr, (bad, r.stderr)
    r = _run(base + ["--backend", "omp", "--frames"], tmp_path)
    assert r.returncode == 1 and "--frames" in r.stderr
    refused = [
        (["--gpus", 2], "--gpus"),
        (["--server", "/nowhere.sock"], "--server"),
        (["--bench", 4], "--bench"),
        (["--backend", "auto"], "--backend auto"),
        (["--checkpoint-every", 2], "--checkpoint-every"),
        (["--converge-every", 2], "--converge-every"),
    ]
    for extra, name in refused:
        r = _run(base + ["--frames", 2] + extra, tmp_path)
        assert r.returncode == 1 and name in r.stderr and "--frames" in r.stderr, (extra, r.stderr)
    r = _run(["--help"], tmp_path)
    assert r.returncode == 0 and "--frames N" in r.stdout


# ---- latency model -------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swar_model.json")


def test_swar_model_batch_default_is_the_single_image(native):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for g in golden["geometries"]:
        args = (g["steps"], g["channels"], g["rows"], g["row_bytes"])
        assert native.swar_model(*args) == native.swar_model(*args, batch=1), args
        assert native.swar_model_table(*args) == native.swar_model_table(*args, batch=1), args
    with pytest.raises(RuntimeError, match="batch"):
        native.swar_model(8, "grey", 64, 64, batch=0)


def test_swar_model_batch_bounds(native):
    """cycles(1) <= cycles(B) <= B * cycles(1) for every shape: the workgroups
    per CU are ceil(B * tiles / 256) <= B * ceil(tiles / 256) (ceil is
    subadditive), the cost per round does not fall as a CU fills, and the
    launch constant is paid once instead of B times."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    geoms = [(g["steps"], g["channels"], g["rows"], g["row_bytes"]) for g in golden["geometries"]]
    geoms += [(8, "grey", 630, 1920), (8, "rgb", 630, 5760), (1, "rgba", 70, 400)]
    for args in geoms:
        one = native.swar_model_table(*args)
        if any(t[5] for t in one):
            pytest.skip("a device is present: the model uses measured kernel resources")
        for b in (2, 7, 64):
            many = native.swar_model_table(*args, batch=b)
            assert [t[:5] for t in many] == [t[:5] for t in one]
            for t1, tb in zip(one, many):
                if t1[6] >= 1e299:  # the shape cannot run these steps, whatever the batch
                    assert tb[6] >= 1e299
                    continue
                assert t1[6] <= tb[6] * (1 + 1e-12) and tb[6] <= b * t1[6] * (1 + 1e-12), (args, b, t1[:3])
            # the pick is the table's cheapest row
            pick, cycles = native.swar_model(*args, batch=b)
            assert cycles == pytest.approx(min(t[6] for t in many), rel=1e-12)
