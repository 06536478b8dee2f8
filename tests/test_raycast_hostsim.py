"""The ray-cast kernels of csrc_cast/ on the host simulator against tests/raycast_oracle.py, bit for bit on the depth, the
normals, the colours and the shade (tests/_raycast_cases.py: the cases, the cull's exactness, batches, NULL outputs; the
simulator's guard bands round every array are the guard rows), and the analytic checks of the oracle itself."""
import numpy as np
import pytest

import _hostsim_cast as HC
import _raycast_cases as RC
import raycast_oracle as RO


class Backend:
    @staticmethod
    def brick_mask(planes, min_weight):
        return HC.brick_mask(planes, min_weight)

    @staticmethod
    def cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight, mask, normals, colour, shade):
        return HC.cast(planes, origin, voxel, view, hw, near, step, n_steps, min_weight, mask, normals, colour, shade)


def test_the_cases_are_the_listed_ones():
    assert tuple(RC.cases()) == RC.NAMES


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_equals_the_oracle_bit_for_bit(name):
    ref = RC.check(name, Backend)
    case = RC.cases()[name]
    if not case["hits"]:
        return
    assert ref["hit"].any() and (ref["depth"][ref["hit"]] > 0).all()


def test_cases_without_a_surface_are_all_zero():
    for name in ("empty", "thin_x", "one_step", "sphere_inside"):
        ref = RC.reference(name)
        assert not ref["hit"].any()
        for key in RC.KEYS:
            assert not ref[key].any(), (name, key)
    # the spoiled records (a NaN, 1e30) and the views that miss the box or look away give nothing either
    assert not RC.reference("axis_nan_huge")["hit"][1:].any() and not RC.reference("outside_box")["hit"][1:].any()
    assert not RC.reference("behind_back_face")["hit"][0].any()


def test_views_equal_the_oracle():
    rng = np.random.default_rng(5)
    c2w = rng.standard_normal((5, 3, 4)) * np.array([1, 1, 1, 1e3])
    c2w[2, 1, 3], c2w[3, 0, 0] = 1e-320, np.pi
    got = HC.views(c2w, RC.K)
    assert RC.same_bits(got, RO.views(c2w, RC.K))
    assert got[0, 12] == 12 and got[0, 14] == 9.5 and got[0, 15] == 5.5


def test_views_in_batches():
    RC.check_batches(Backend)


def test_null_outputs():
    RC.check_null_outputs(Backend)


def test_a_mask_that_marks_nothing_gives_no_hit_where_the_oracle_has_one():
    """the mask is read: with no brick marked (not a mask the header allows) nothing is evaluated and nothing is hit, so
    the equalities above are not those of a kernel that ignores its mask"""
    case = RC.cases()["plane"]
    mask = np.zeros_like(RC.reference("plane")["mask"])
    got = RC._cast(case, Backend, mask=mask)
    assert RC.reference("plane")["hit"].any() and not got["depth"].any() and not got["shade"].any()


def test_analytic_plane():
    """The oracle's depth on the fused plane against the rays' true depth, and the shade of the central pixels.

    Measured on the oracle (printed below): the largest depth error over the hits of both views is 2.1e-07 (fp32 rounding:
    the fused tsdf is linear in z across the band, so the interpolated crossing is exact up to rounding); asserted
    at four times that.  The central pixels of the fusing view look along the plane's normal to within atan(3 / 12), where
    255 cos is 247.4 .. 254.9: the oracle's bytes span 248 .. 255, and that spread is the assertion."""
    err = RC.plane_depth_error()
    shade = RC.plane_central_shade()
    print(f"plane: largest depth error {err:.3e}; central shade {shade.min()} .. {shade.max()}")
    assert err <= 4 * 2.1e-07
    assert shade.min() >= 248 and shade.max() == 255


def test_analytic_sphere():
    """The oracle's depth and normal on the analytic sphere against the ray-sphere intersection and the radial direction.

    Measured on the oracle (printed below): the largest depth error is 2.8e-02 (0.28 voxels, at the grazing rays of the
    limb: trilinear interpolation of a distance field of radius 5 voxels, sampled every voxel along the ray) and the
    largest angle between the normal and the radius is 1.4e-01 rad; asserted at four times those."""
    depth_err, angle = RC.sphere_errors()
    print(f"sphere: largest depth error {depth_err:.3e}, largest normal angle {angle:.3e} rad")
    assert depth_err <= 4 * 2.8e-02
    assert angle <= 4 * 1.4e-01
