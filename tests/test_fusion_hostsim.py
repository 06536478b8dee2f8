"""libscsfm_fuse.so's kernels on the host simulator (tests/_hostsim_fuse.py) against tests/fusion_oracle.py, bit for bit:
the cases of tests/_fusion_cases.py, which tests/test_gpu_fusion.py runs on the device.  The oracle tests every voxel
against every frame, so equal bits on the cases whose tiles straddle a frustum show that the kernels' cull is conservative."""
import numpy as np
import pytest

import _fusion_cases as C
import _hostsim_fuse as HF
import fusion_oracle as O


class Backend:
    @staticmethod
    def volume(dims, origin, voxel, trunc, max_weight, frames_per_launch):
        return HF.Volume(dims, origin, voxel, trunc, max_weight, frames_per_launch)

    @staticmethod
    def set_planes(vol, planes):
        vol.planes[...] = planes

    dev = staticmethod(lambda a: a)
    host = staticmethod(lambda a: a)

    @staticmethod
    def extract_guarded(vol, min_weight, capacity):
        return vol.extract(min_weight, capacity)  # (between guard bands, which the call checks)


@pytest.mark.parametrize("name", C.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    _, n = C.check(name, Backend)
    assert (n == 0) == (name == "empty")


def test_the_cases_exercise_what_they_are_for():
    """the oracle alone: tiles wholly unseen next to tiles partly seen (a frustum plane cuts them), a weight at its cap,
    depths rejected, both zeros on crossings' ends"""
    ref = C.reference("straddle_F5")[0]
    nx, ny, nz = ref.dims
    seen = ref.weight > 0
    kinds = set()
    for z0 in range(0, nz, 4):
        for y0 in range(0, ny, 8):
            for x0 in range(0, nx, 32):
                tile = seen[z0:z0 + 4, y0:y0 + 8, x0:x0 + 32]
                kinds.add("none" if not tile.any() else ("all" if tile.all() else "part"))
    assert kinds >= {"none", "part"}, kinds
    capped = C.reference("max_weight")[0]
    assert capped.weight.max() == 3.0 and (capped.weight == 3.0).sum() > 50
    clean, dirty = C.reference("straddle_F5")[0], C.reference("dirty_depth")[0]
    assert dirty.weight.sum() > 0 and np.isfinite(dirty.planes).all()
    assert np.isfinite(C.reference("dirty_disp")[0].planes).all() and clean.weight.sum() > 0
    zeros = C.reference("signed_zeros")
    a = O.Volume.crossings(zeros[0], 2.0)[0]
    t = zeros[0].tsdf.reshape(-1)
    ends = t[np.concatenate([a, a + 1])]
    assert ((ends == 0) & ~np.signbit(ends)).any() and ((ends == 0) & np.signbit(ends)).any()
    assert 0 < len(C.reference("min_weight_2")[1]) < C.reference("min_weight_2")[0].count(1.0)
    assert not C.reference("no_image_alone")[0].colour.any() and C.reference("no_image")[0].colour.any()
    assert len(C.reference("chunk_x")[1]) > 20


def test_capacity_below_and_at_the_count():
    C.check_capacity("straddle_F5", Backend)


def test_cameras_equal_the_oracle():
    case = C.cases()["straddle_F8_vec"]["calls"][0]
    got, want = HF.cameras(case["c2w"], C.K), O.cameras(case["c2w"], C.K)
    assert C.same_bits(got, want)
    # against numpy's inverse, to rounding
    full = np.concatenate([case["c2w"], np.tile([[[0, 0, 0, 1.0]]], (8, 1, 1))], axis=1)
    inv = np.linalg.inv(full)
    assert np.allclose(got[:, :9].reshape(-1, 3, 3), inv[:, :3, :3], atol=1e-6)
    assert np.allclose(got[:, 9:12], inv[:, :3, 3], atol=1e-5)


def test_analytic_plane():
    """A fronto-parallel plane at depth D0 = 1.73 seen by three cameras with identity rotation: every point on a z-edge
    lies within four times the oracle's own largest deviation from D0, and at least 90 % of the in-frustum columns yield
    a point -- for the oracle alone, then for the kernels.

    Measured (host simulator and oracle, which agree bit for bit): largest |z - D0| 1.907e-08 for both -- every z is the
    float nearest to 1.73 --, every in-frustum column (100 %) with a point."""
    ref, xyz, _, axis = C.analytic_reference()
    dev_ref, share_ref = C.plane_statistics(xyz, axis)
    print(f"oracle: largest |z - D0| {dev_ref:.3e}, share of the in-frustum columns with a point {share_ref:.3f}")
    assert share_ref >= 0.9 and (axis == 2).sum() > 100
    vol = HF.Volume(**C.ANALYTIC)
    vol.integrate(**C.analytic_call())
    got_xyz, _ = vol.extract(1.0)
    assert len(got_xyz) == len(xyz)
    dev, share = C.plane_statistics(got_xyz, axis)
    print(f"kernels: largest |z - D0| {dev:.3e}, share {share:.3f}")
    assert dev <= 4 * dev_ref and share >= 0.9
    assert C.same_bits(got_xyz, xyz) and C.same_bits(vol.planes, ref.planes)
