"""CPU: gsm::AttributeValue / AttributeInRange / AttributeBin / FloatToSortableUint (csrc/gs_device_math.h) compiled for the host with tests/harness.py's
line and run per splat by tests/attribute_host_harness.cpp, held to the numpy twin bit for bit and integer for integer on the adversarial family of
tests/attribute_rig.py and on every preset's decode; and the same program under the host sanitizers."""
import subprocess

import numpy as np
import pytest

import attribute_model as AM
import attribute_rig as AR
from builders import decode_of
from common import PRESETS, small_asset
from harness import build_harness, run_under_sanitizers

f32 = np.float32


@pytest.fixture(scope="module")
def attr_harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("attributes"), "attribute_host_harness.cpp", exe=True)


def host_run(exe, tmp_path, asset, attr, point, lo, hi, bins):
    """(value words, keys, histogram words, in-range flags) of every splat of the asset"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    blobs = [np.ascontiguousarray(b, np.uint8) if b is not None else np.zeros(0, np.uint8) for b in (asset.posData, asset.otherData, asset.colorData, asset.shData, asset.chunkData)]
    s = AM.hist_scale(lo, hi, bins) if bins else f32(0.0)
    head = np.array([asset.splatCount, int(asset.posFormat), int(asset.scaleFormat), int(asset.colorFormat), int(asset.shFormat), len(blobs[4]) // 64, attr, bins], np.uint32)
    with open(src, "wb") as f:
        f.write(head.tobytes() + np.array(list(point) + [lo, hi, s], f32).tobytes() + np.array([len(b) for b in blobs], np.uint64).tobytes())
        for b in blobs:
            f.write(b.tobytes())
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = np.fromfile(dst, np.uint32).reshape(-1, 4)
    return got[:, 0], got[:, 1], got[:, 2], got[:, 3]


def check(exe, tmp_path, asset, dec, what, bins_list):
    for attr in AM.ATTRS:
        v = AM.values(dec, attr, AR.POINT)
        for bins in bins_list:
            words, keys, hist, inside = host_run(exe, tmp_path, asset, attr, AR.POINT, AR.HIST_LO, AR.HIST_HI, bins)
            assert AM.same_words(words, v).all(), (what, attr, np.flatnonzero(~AM.same_words(words, v))[:8])
            num = ~np.isnan(v)
            assert np.array_equal(keys[num], AM.keys(v)[num]), (what, attr)
            assert np.array_equal(hist, AM.bin_of(v, AR.HIST_LO, AR.HIST_HI, bins)), (what, attr, bins, np.flatnonzero(hist != AM.bin_of(v, AR.HIST_LO, AR.HIST_HI, bins))[:8])
            assert np.array_equal(inside.astype(bool), AM.in_range(v, AR.HIST_LO, AR.HIST_HI)), (what, attr)


def test_host_values_bins_and_keys_equal_the_twin_on_the_adversarial_family(attr_harness, tmp_path):
    fields = AR.adversarial()
    check(attr_harness, tmp_path, AR.attribute_asset(*fields), AR.fields_of(*fields), "adversarial", AR.FAMILY_BINS)


@pytest.mark.parametrize("quality", PRESETS)
def test_host_values_equal_the_twin_on_every_preset(attr_harness, tmp_path, quality):
    # (a Cluster* SH table needs more splats than entries: those two presets at the 20,000 whose decode the GPU suites share)
    n = 20000 if quality in ("VeryLow", "Low") else 700
    check(attr_harness, tmp_path, small_asset(n, 5, quality), decode_of(n, quality), quality, (64,))


def test_ranges_at_infinite_and_inverted_bounds(attr_harness, tmp_path):
    fields = AR.adversarial()
    asset, dec = AR.attribute_asset(*fields), AR.fields_of(*fields)
    v = AM.values(dec, AM.VOLUME)
    for lo, hi in ((-np.inf, np.inf), (0.75, 0.25), (-0.0, 0.0), (np.inf, np.inf)):
        inside = host_run(attr_harness, tmp_path, asset, AM.VOLUME, AR.POINT, lo, hi, 0)[3]
        assert np.array_equal(inside.astype(bool), AM.in_range(v, lo, hi)), (lo, hi)
    assert host_run(attr_harness, tmp_path, asset, AM.VOLUME, AR.POINT, -np.inf, np.inf, 0)[3].sum() == (~np.isnan(v)).sum()
    assert not host_run(attr_harness, tmp_path, asset, AM.VOLUME, AR.POINT, 0.75, 0.25, 0)[3].any()


def test_host_harness_under_the_sanitizers(tmp_path):
    """the stand-alone program over its own input (NaN and +-0 scale triples, an overflowing product, opacities on and beside the range), built with
    ASan and UBSan"""
    out = run_under_sanitizers(tmp_path, "attribute_host_harness.cpp", "ATTRIBUTE_HARNESS_SANITIZED")
    assert out.returncode == 0 and "attribute_host_harness ok" in out.stdout, out.stderr[-2000:]
