"""The size lists, frames and expected-destination contract that
tests/test_gpu_single_step.py takes from tests/tile_edges.py, checked without a
GPU: every lane, workgroup and row-march edge of k_binomial / k_generic9 the
GPU file claims to run is in the lists."""
import numpy as np
import pytest

import tile_edges as te


@pytest.mark.parametrize("c", [1, 3, 4])
def test_widths_hold_every_lane_and_workgroup_edge(c):
    rbs = [w * c for w in te.single_step_widths(c)]
    assert rbs == sorted(set(rbs)) and rbs[0] == c and 2 * c in rbs
    valids = {rb % te.LANE or te.LANE for rb in rbs}
    # a row of whole RGBA pixels ends on a multiple of 4 bytes: 4 and 12 are its 1 and 15
    lo, hi = te.partial_valids(c)
    assert (lo, hi) == ((1, 15) if c != 4 else (4, 12))
    assert {lo, hi, te.LANE} <= valids
    for edge in (te.LANE, 2 * te.LANE, te.WG_BYTES, 2 * te.WG_BYTES):
        below, above = [rb for rb in rbs if rb < edge], [rb for rb in rbs if rb > edge]
        assert edge - max(below) <= c and min(above) - edge <= c, "no whole-pixel width beside the edge"
        assert (edge in rbs) == (edge % c == 0)
    # the 1024-byte seam from both sides, and three workgroups in x
    assert any(te.WG_BYTES - c <= rb < te.WG_BYTES for rb in rbs) and any(te.WG_BYTES < rb for rb in rbs)
    assert -(-max(rbs) // te.WG_BYTES) >= 3 and max(rbs) >= 2049
    if c == 3:  # the last pixel across two lanes (bytes 30..32) and across the seam (1023..1025)
        assert 11 in te.single_step_widths(c) and 342 in te.single_step_widths(c)
        assert 33 - c < 2 * te.LANE < 33 and 342 * c - c < te.WG_BYTES < 342 * c


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("kernel", ["binomial", "generic9"])
def test_sizes_pair_every_width_and_height(kernel, c):
    sizes = te.single_step_sizes(kernel, c)
    hs = te.SINGLE_STEP_HEIGHTS[kernel]
    assert hs == ((1, 2, 3, 4, 5, 15, 16, 17, 33) if kernel == "binomial" else (1, 2, 3, 4, 5, 9))
    assert len(sizes) == len(set(sizes))
    assert {h for h, _ in sizes} == set(hs) and {w for _, w in sizes} == set(te.single_step_widths(c))
    # the seam widths at every small height; the tall heights past the seam and at three workgroups
    seam = te.seam_widths(c)
    assert len(seam) >= 2 and min(seam) * c < te.WG_BYTES < max(seam) * c
    for w in seam:
        assert {h for h in hs if h <= 5} <= {h for h, ww in sizes if ww == w}
    for w in (max(seam), max(te.single_step_widths(c))):
        assert {h for h in hs if h > 5} <= {h for h, ww in sizes if ww == w}
    # more than one workgroup in y, and a last row group that is partial
    rows = te.WG_ROWS[kernel]
    assert any(h > rows and h % rows for h, _ in sizes)
    # paired, not multiplied out; the largest frame is about 2100 bytes x 33 rows
    assert len(sizes) < len(hs) * len(te.single_step_widths(c)) // 2
    assert max(h for h, _ in sizes) <= 33 and max(w * c for _, w in sizes) <= 2100


def _lay(rb, rows, halo):
    pitch = te.PAD + -(-rb // 16) * 16 + 16
    return {"row_bytes": rb, "rows": rows, "pitch": pitch, "bytes": (rows + 2 * halo) * pitch}


@pytest.mark.parametrize("rb", [1, 15, 16, 17, 33, 1026])
def test_expected_tail_zeros_differs_only_in_the_tail(rb):
    halo, rows, lo, hi = 2, 5, 1, 4
    lay = _lay(rb, rows, halo)
    shape = (rows + 2 * halo, lay["pitch"])
    ref = np.full((hi - lo, rb), 7, np.uint8)
    plain = te.expected(shape, lay, halo, ref, lo, hi)
    tail = te.expected(shape, lay, halo, ref, lo, hi, tail_zeros=True)
    assert np.array_equal(plain, te.expected(shape, lay, halo, ref, lo, hi, tail_zeros=False))
    diff = np.flatnonzero(plain != tail)
    up = -(-rb // 16) * 16
    want = [te.GUARD + (halo + r) * lay["pitch"] + te.PAD + x for r in range(lo, hi) for x in range(rb, up)]
    assert diff.tolist() == want
    assert (tail[diff] == 0).all() and (plain[diff] == te.CANARY).all()
    # nothing is launched: all canary either way
    assert (te.expected(shape, lay, halo, ref[:0], 3, 3, tail_zeros=True) == te.CANARY).all()


def test_zero_pad_frames():
    halo, rows, rb = 3, 4, 21
    lay = _lay(rb, rows, halo)
    img = np.arange((rows + 2 * halo) * rb, dtype=np.uint8).reshape(-1, rb) | 1
    clean, dirty = te.frames(lay, halo, img, 2, 1, pads="zero")
    old_clean, old_dirty = te.frames(lay, halo, img, 2, 1)
    assert np.array_equal(clean, old_clean)
    assert (old_dirty[:, :te.PAD] == 0xFF).all() and (old_dirty[:, te.PAD + rb:] == 0xFF).all()  # the default
    assert (dirty[:2] == 0xFF).all() and (dirty[-1:] == 0xFF).all()    # outside the image: end to end
    inside = dirty[2:-1]
    assert not inside[:, :te.PAD].any() and not inside[:, te.PAD + rb:].any()
    assert np.array_equal(inside[:, te.PAD:te.PAD + rb], img[2:-1])


@pytest.mark.parametrize("c", [1, 3, 4])
def test_images(c):
    rb = (te.WG_BYTES // c + 1) * c
    lo, hi = te.half_lane_stripes(3, rb, True), te.half_lane_stripes(3, rb, False)
    assert np.array_equal(lo ^ hi, np.full((3, rb), 255, np.uint8))
    assert lo[0, :16].tolist() == [255] * 8 + [0] * 8
    cols = te.untouched_zero_columns(hi, c)
    assert cols.any() and not hi[:, cols].any()
    x = np.flatnonzero(cols)
    assert all((xx - c < 0 or hi[0, xx - c] == 0) and (xx + c >= rb or hi[0, xx + c] == 0) for xx in x)
    seen = set()
    for flip in (False, True):
        img, n = te.impulses(5, rb, c, flip)
        ys, xs = np.nonzero(img)
        assert n >= 4 and len(ys) == n * c and set(ys) == {0, 4}
        px = sorted({(int(y), int(b) // c) for y, b in zip(ys, xs)})
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3 for i, a in enumerate(px) for b in px[i + 1:])
        seen |= {int(b) for y, b in zip(ys, xs) if y == 0}
    # between the two images row 0 holds both sides of the seam and of a lane edge
    assert {te.WG_BYTES - 1, te.WG_BYTES, te.LANE - 1, te.LANE, 0, rb - 1} <= seen
    taps = [3, 1, 0, 2, 5, 1, -1, 2, 4]
    s = te.exact_sums(te.impulses(5, rb, c)[0], c, taps)
    assert s.min() == -255 and s.max() == 5 * 255
