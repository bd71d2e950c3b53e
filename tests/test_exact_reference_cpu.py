"""exact_gaussian (tests/exact_reference.py, int64) against pconv.numpy_convolve
for both depths and both borders, on uniform random data and on the adversarial
pattern with saturated blocks, checkerboards and column groups: pins the
package's oracle to exact arithmetic at saturated values.  No GPU."""
import numpy as np
import pytest

from exact_reference import adversarial, exact_gaussian

SIZES = [(1, 1), (1, 7), (7, 1), (23, 31)]
STEPS = (1, 2, 5, 16)


def _shape(h, w, c):
    return (h, w, c) if c > 1 else (h, w)


@pytest.mark.parametrize("border", ["zero", "replicate"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_exact_gaussian_equals_numpy_convolve(pconv_mod, channels, dtype, border):
    c = channels
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(9001 + 10 * c + top % 7 + len(border))
    for h, w in SIZES:
        uniform = rng.integers(0, top + 1, size=(h, w * c), dtype=dtype)
        for name, flat in (("uniform", uniform), ("adversarial", adversarial(rng, h, w * c, c, dtype))):
            img = flat.reshape(_shape(h, w, c))
            for steps in STEPS:
                got = exact_gaussian(img, steps, border)
                ref = pconv_mod.numpy_convolve(img, steps, "gaussian", border)
                assert got.dtype == dtype and got.shape == img.shape
                assert np.array_equal(got, ref), (name, h, w, steps)


def test_hand_worked_values():
    """The reference itself, against values worked by hand."""
    one = np.array([[255]], np.uint8)
    assert exact_gaussian(one, 1, "zero")[0, 0] == (4 * 255) >> 4  # 63
    assert exact_gaussian(one, 1, "replicate")[0, 0] == 255  # a constant image is a fixed point
    assert exact_gaussian(np.full((5, 6, 3), 65535, np.uint16), 16, "replicate").min() == 65535
    x = np.array([[0, 16, 0]], np.uint8)  # one row: only the middle row of weights sees data
    assert exact_gaussian(x, 1, "zero").tolist() == [[2, 4, 2]]
    assert exact_gaussian(x, 1, "replicate").tolist() == [[4, 8, 4]]  # rows above and below replicate: x4 per column
    rgb = np.zeros((1, 2, 3), np.uint8)
    rgb[0, 0] = (16, 32, 64)  # channels never mix
    assert exact_gaussian(rgb, 1, "zero").tolist() == [[[4, 8, 16], [2, 4, 8]]]
    with pytest.raises(TypeError):
        exact_gaussian(np.zeros((2, 2), np.int32), 1, "zero")


def test_adversarial_pattern_holds_its_plants():
    for dtype in (np.uint8, np.uint16):
        top = int(np.iinfo(dtype).max)
        a = adversarial(np.random.default_rng(1), 37, 53 * 3, 3, dtype)
        assert a.dtype == dtype and a.shape == (37, 159)
        assert (a[7:11, 22:31] == top).all()  # the saturated block
        assert a[18, :79].tolist() == [(x & 1) * top for x in range(79)]  # the checkerboard
        # column groups of 3 samples: byte 53 is the last of pixel 17 (odd: 0), then pixel 18 (max), 19, 20
        assert a[27, 53:63].tolist() == [0] + [top] * 3 + [0] * 3 + [top] * 3
