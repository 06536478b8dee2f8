"""libscsfm_conf.so's kernels on the host simulator (tests/_hostsim_conf.py) against tests/confidence_oracle.py, bit for
bit: the cases of tests/_conf_cases.py, which tests/test_gpu_confidence.py runs on the device.  Then, on the oracle alone,
that the constructed cases exercise the rule each is for, and that the confidence does its job on a generated world with
an object that moves against the poses."""
import numpy as np
import pytest

import _conf_cases as C
import _hostsim_conf as HC
import _hostsim_fuse as HF
import confidence_oracle as CO

f32 = np.float32


class Backend:
    pairs = staticmethod(HC.pairs)
    weights = staticmethod(HC.weights)
    dev = staticmethod(lambda a: a)
    host = staticmethod(lambda a: a)

    @staticmethod
    def volume(dims, origin, voxel, trunc, max_weight, frames_per_launch):
        return HC.Volume(dims, origin, voxel, trunc, max_weight, frames_per_launch)


@pytest.mark.parametrize("name", C.NAMES)
def test_weights_equal_the_oracle_bit_for_bit(name):
    C.check(name, Backend)


@pytest.mark.parametrize("name", C.FUSE_NAMES)
def test_integration_equals_the_oracle_bit_for_bit(name):
    """at F, 2 and 1 frames a launch and as F calls of one frame; a weight of all ones also against libscsfm_fuse's own
    kernels (tests/_hostsim_fuse.py) over all five planes"""
    ref = C.check_fuse(name, Backend)
    assert ref.weight.max() > 2 and np.isfinite(ref.planes).all()


@pytest.mark.parametrize("kind", ("rigid", "skewed"))
def test_pairs_equal_the_oracle_and_numpy(kind):
    c2w = C.pair_poses()[kind]
    n = len(c2w)
    full = np.concatenate([c2w, np.tile([[[0, 0, 0, 1.0]]], (n, 1, 1))], axis=1)
    for radius in (1, 2, 4):
        got, want = HC.pairs(c2w, C.K_ODD, radius), CO.pairs(c2w, C.K_ODD, radius)
        assert got.shape == (n, 2 * radius, 16) and C.same_bits(got, want)
        for i in range(n):
            for s, o in enumerate(CO.offsets(radius)):
                if 0 <= i + o < n:
                    rel = np.linalg.inv(full[i + o]) @ full[i]      # frame i's camera to frame j's
                    assert np.allclose(got[i, s, :9].reshape(3, 3), rel[:3, :3], atol=1e-6)
                    assert np.allclose(got[i, s, 9:12], rel[:3, 3], atol=1e-6)
                    assert got[i, s, 12:].tolist() == [37.0, 37.0, 29.5, 17.5]
                else:
                    assert not got[i, s].view(np.uint32).any()      # sixteen zeros, by bits (no -0.0)
    assert [CO.offsets(r) for r in (1, 2)] == [[-1, 1], [-2, -1, 1, 2]]


def test_the_cases_exercise_what_they_are_for():
    """the oracle alone, one rule after another"""
    H, W = C.HW
    # a whole pixel towards either neighbour: u is an integer; x0 = W - 2 counts and x0 = W - 1 does not; v = py puts y0 on
    # the last row, which has no row below it
    _, w, count = C.reference("integer_x")
    want = np.zeros((H, W), int)
    want[:H - 1] = (np.arange(W) - 1 >= 0) * 1 + (np.arange(W) + 1 <= W - 2) * 1
    assert np.array_equal(count[1], want) and want[0, W - 1] == 1 and want[0, W - 2] == 1 and want[0, 0] == 1
    assert (w[count > 0] == 1).all()
    _, _, count = C.reference("integer_y")
    want = np.zeros((H, W), int)
    want[:, :W - 1] = ((np.arange(H) - 1 >= 0) * 1 + (np.arange(H) + 1 <= H - 2) * 1)[:, None]
    assert np.array_equal(count[1], want) and want[H - 1, 0] == 1 and want[H - 2, 0] == 1
    # 0.3 of a pixel: u = -0.3 in column 0 is skipped, not truncated to 0 (which would count two)
    _, _, count = C.reference("fraction_x")
    assert (count[1, :H - 1, 0] == 1).all() and (count[1, :H - 1, 1:W - 1] == 2).all() and (count[1, :H - 1, W - 1] == 1).all()
    # own depth 0, NaN, beyond max_depth, negative; disparity 0, NaN, one whose reciprocal overflows
    _, w, count = C.reference("own_depth")
    assert not w[1, 2, 3:7].any() and not count[1, 2, 3:7].any() and w[1, 2, 7] == 1 and w[1, 3, 3] == 1
    _, w, count = C.reference("own_disp")
    assert C.cases()["own_disp"]["depth"][1, 2, 3] == 0 and not w[1, 2, 3:6].any() and w[1, 2, 6] == 1
    # a tap that is 0 (in frame 2) or NaN (in frame 0) costs the four pixels of frame 1 round it that neighbour; in its own
    # frame only the pixel itself, whose own depth it is, loses anything
    for name in ("taps", "taps_disp"):
        base, got = C.reference("fraction_x")[2], C.reference(name)[2]
        lost = base - got
        assert lost.min() == 0 and lost[1].sum() == 8 and lost[1].max() == 1, name
        assert np.argwhere(lost[0]).tolist() == [[8, 12]] and np.argwhere(lost[2]).tolist() == [[5, 7]], name
    # every neighbour behind the camera
    assert not C.reference("behind")[2].any() and not C.reference("behind")[1].any()
    # one frame has no neighbour; two frames at radius 4 have one present slot of eight
    assert not C.reference("n1_r1_w4_depth")[1].any() and not C.reference("n1_r1_odd_disp")[0].any()
    pair = C.reference("n2_r4_odd_depth")[0]
    assert [(pair[i, :, 12] > 0).tolist() for i in range(2)] == [[0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0]]
    # min_views = 2: the two end frames have one neighbour, and pixels with one valid neighbour lose their weight
    plain, two = C.reference("n5_r1_w4_depth"), C.reference("min_views_2")
    assert not two[1][0].any() and not two[1][4].any() and two[1][1:4].any()
    assert ((plain[2] == 1) & (plain[1] > 0)).any() and not two[1][plain[2] == 1].any()
    assert C.same_bits(two[1][plain[2] == 2], plain[1][plain[2] == 2])
    # the floor cuts some pixels and not others, and leaves the others' bits
    plain, cut = C.reference("n5_r2_odd_depth")[1], C.reference("floor")[1]
    gone = (plain > 0) & (cut == 0)
    assert 100 < gone.sum() < (plain > 0).sum() - 100 and (plain[gone] < f32(0.99)).all() and (cut[cut > 0] >= f32(0.99)).all()
    assert C.same_bits(cut[~gone], plain[~gone])
    # max against mean on the same input
    best = C.reference("max")[1]
    assert (best >= plain).all() and (best > plain).sum() > 1000
    # both values of is_disp see the same world
    assert np.allclose(C.reference("n5_r2_odd_disp")[1], plain, atol=1e-5)


def test_identical_frames_at_identical_poses_weigh_exactly_one():
    for name in ("identical", "identical_pow2"):
        _, w, count = C.reference(name)
        assert (count > 0).sum() > 500 and (w[count > 0] == f32(1)).all(), name
        got = HC.weights(C.cases()[name]["depth"], HC.pairs(C.cases()[name]["c2w"], C.cases()[name]["K"], 1),
                         **C.cases()[name]["kw"])
        assert (got[count > 0] == f32(1)).all() and not got[count == 0].any()


def test_skipped_weights_are_skipped():
    """on the oracle: weights of 0, -1, NaN, 1.5 and the float above 1 behave as a depth of 0 at those pixels does"""
    case = C.fuse_cases()["skips_scalar_image"]
    w = case["weight"]
    bad = ~((w > 0) & (w <= 1))
    assert bad.sum() > 100 and np.isnan(w).any() and (w == 1.5).any() and (w == 0).any() and (w == -1).any()
    call = dict(case["call"])
    call["depth"] = np.where(bad, f32(0), call["depth"])
    vol = CO.Volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"])
    vol.integrate(**call, weight=np.where(bad, f32(0.5), w))
    ref = C.fuse_reference("skips_scalar_image")
    assert C.same_bits(vol.planes, ref.planes)
    full = CO.Volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"])
    full.integrate(**case["call"], weight=np.where(bad, f32(0.5), w))
    assert not C.same_bits(full.planes, ref.planes)
    # a max_weight that w + c crosses with a fractional c
    capped = C.fuse_reference("max_weight_scalar_image")
    assert capped.weight.max() == 2.5 and (capped.weight == 2.5).sum() > 50
    frac = capped.weight[(capped.weight > 0) & (capped.weight < 2.5)]
    assert (frac != np.round(frac)).any()


def test_weighted_integration_on_the_simulator_equals_the_unweighted_library():
    """the weight-1 test that keeps csrc_conf's restated kernel in step with csrc_fuse's: the two libraries, on the
    simulator, over all five planes"""
    case = C.fuse_cases()["ones_vector_image"]
    call = case["call"]
    a = HC.Volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"], 8)
    b = HF.Volume(case["dims"], case["origin"], case["voxel"], None, case["max_weight"], 8)
    a.integrate(**call, weight=case["weight"])
    b.integrate(**call)
    assert b.weight.max() == 3 and C.same_bits(a.planes, b.planes)


def test_confidence_does_its_job_on_the_oracle():
    """A static height field, six 37 x 61 frames with true poses and 1 % noise on the depth, and in every frame a plate of
    8 x 8 pixels that comes 0.1 nearer from frame to frame.  Conditions: the median weight on the plates is below the
    median weight on the static pixels that have a neighbour; fusing with the floor half way between the two medians
    leaves fewer surface points (min_weight 2) inside the object's swept box than unweighted fusion and at least 0.9
    times as many outside it.

    Measured on the oracle: medians 0.959177 (plates) and 0.995635 (static), floor 0.977406; points inside the box 104
    unweighted and 0 weighted, outside it 2257 and 2164."""
    m = C.moving_reference()
    on, off = m["medians"]
    print(f"medians: plates {on:.6f}, static {off:.6f}; floor {m['floor']:.6f}; points (inside, outside): unweighted "
          f"{m['plain']}, weighted {m['weighted']}")
    assert C.moving_world()["patch"].sum() == 6 * 64
    assert on < off and on < m["floor"] < off
    assert m["weighted"][0] < m["plain"][0] and m["weighted"][1] >= 0.9 * m["plain"][1]
    # and the kernels give the oracle's weights on this world
    w = C.moving_world()
    got = HC.weights(w["depth"], HC.pairs(w["c2w"], w["K"], 1), is_disp=False, max_depth=C.MAX_DEPTH, floor=m["floor"])
    assert C.same_bits(got, m["cut"])
