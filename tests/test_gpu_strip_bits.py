"""The strip gather (ba_gather128s_kernel, csrc/gather128s.hip) against recorded bits.

tests/golden/strip_parent_bits.npz holds what the build of commit d44889b ("Gather: launches from plan_gather_steps, one copy of
shared helpers") computed on an MI355X for the cases of tools/record_strip_bits.py: AtA, Atb, absres, nvalid and the mask of
ops.ba_assemble(..., return_mask=True) and the per-pixel records the gather hands to the SYRK (large arrays strided, see
subsample() there).  That build ran every cross-lane reduction of the kernel's lane = pixel phases (row statistics, the plan's
window extent, the per-slice sum|d| fold) as a __shfl_xor butterfly; the kernel now uses DPP and the half / row swaps with
the same pairing, and whatever else changes in the phases outside the slice loop has to keep the bits too.

Shapes: 21 wide (the narrowest map the rolling window fits) x 24 (one whole and one ragged segment), its transpose 24 x 21,
40 x 37 (ragged strips and segments), 64 x 48 x 2 windows.  Forms: K = 0 / 128 / 256; 1 and 4 target frames, the latter as
frame-parallel workgroups and as a loop inside one wave (same bits, one record); 8-, 16- and 32-row segments; every row on the
window-less path; scenes with large motion and depth steps (pixels outside the image, on its rim, rows too wide for the window).
The inputs come from numpy's Mersenne Twister and IEEE + - * / sqrt only, so every host makes the same bits.

One differential case keeps the file from being the only witness: the strip kernel against ba_gather128_kernel."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tools")) if p not in sys.path]
import record_strip_bits as rsb  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "strip_parent_bits.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", rsb.CASES, ids=[c[0] for c in rsb.CASES])
def test_strip_gather_keeps_the_recorded_bits(case, gold):
    name, W, H, B, K, pairs, extra, big, same_as = case
    got = rsb.run(case, torch.device("cuda:0"))
    ref = same_as or name
    assert set(got) == set(rsb.NAMES) - (set() if K else {"records"})
    for k, v in got.items():
        assert same_bits(v, gold["%s/%s" % (ref, k)]), (name, k)
    if same_as is None:       # the recorded case is worth its bits only if the kernel did something: pixels in the mask, not all of them
        assert 0 < int(got["mask"].sum()) and (got["mask"] <= 1).all()
        assert np.isfinite(got["AtA"]).all() and float(np.abs(got["AtA"]).max()) > 0
        if K:
            assert float(np.abs(got["records"]).max()) > 0


def test_the_file_covers_every_case_and_nothing_else(gold):
    want = {"%s/%s" % (c[0], k) for c in rsb.CASES if c[8] is None for k in rsb.NAMES if c[4] or k != "records"}
    assert set(gold.files) == want


def test_scenes_put_rim_pixels_and_direct_rows_in_play():
    """(host only, counts from a float64 restatement of the geometry) the large-motion scenes have pixels outside the target image, on
    its rim and pixel rows too wide for the window; the calm ones still touch the rim"""
    for c in rsb.CASES:
        out, rim, wide = rsb.scene_stats(c)
        assert rim > 0 and out > 0, c[0]
        if c[7] and c[1] >= 40:
            assert wide > 0, c[0]


def test_strip_gather_matches_the_direct_kernel():
    """ba_gather128s_kernel against ba_gather128_kernel (direct taps, one pixel per 16 lanes): same arithmetic per pixel, the channel
    sums added in another order -> to rounding (the tolerance of tests/test_gpu_round3.py), the in-image mask bit for bit"""
    from banet_amd import _capi as capi
    case = rsb.case_by_name("w40_k128")
    dev = torch.device("cuda:0")
    strip = rsb.run(case, dev)
    direct = rsb.run(case, dev, flags=capi.DEV_DIRECT_GATHER | capi.DEV_NO_STRIP_GATHER)
    relerr = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    for k in ("AtA", "Atb", "absres", "nvalid"):
        print(k, relerr(strip[k], direct[k]))
        assert relerr(strip[k], direct[k]) < 3e-6, k
    assert same_bits(strip["mask"], direct["mask"]) and same_bits(strip["nvalid"], direct["nvalid"])
