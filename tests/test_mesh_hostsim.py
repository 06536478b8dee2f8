"""The mesh kernels (csrc_mesh/scsfm_mesh.hip) on the host simulator against tests/mesh_oracle.py, bit for bit: the cases of
tests/_fusion_cases.py integrated through the simulated fusion library, planes filled by hand, volumes one voxel thick,
the capacities, an analytic sphere (a closed oriented 2-manifold) and two runs with equal bytes."""
import functools

import numpy as np
import pytest

import _fusion_cases as FC
import _hostsim_fuse as HF
import _hostsim_mesh as HM
import _mesh_cases as MC
import mesh_oracle as MO


def _mesh(planes, origin, voxel, min_weight, vcap=None, tcap=None):
    return HM.extract_mesh(planes, origin, voxel, min_weight, vcap, tcap)[:3]


@functools.lru_cache(maxsize=None)
def _fused(name):
    """the case's volume, integrated by the simulated libscsfm_fuse.so (once)"""
    case = FC.cases()[name]
    vol = HF.Volume(case["dims"], case["origin"], case["voxel"], case["trunc"], case["max_weight"])
    if case["planes"] is not None:
        vol.planes[...] = case["planes"]
    for call in case["calls"]:
        vol.integrate(**call)
    return vol


def test_the_fused_volumes_span_whole_and_partial_chunks():
    assert FC.DIMS == (37, 18, 29) and 37 * 18 * 29 == 18 * 1024 + 882  # 19 chunks, the last one partial
    assert sum(FC.cases()[n]["dims"] == FC.DIMS for n in FC.NAMES) >= 9


@pytest.mark.parametrize("name", FC.NAMES)
def test_fusion_cases_equal_the_oracle(name):
    vol = _fused(name)
    triangles = 0
    for min_weight in (1.0, 2.0):
        ref = MO.mesh(vol.planes, vol.origin, vol.voxel, min_weight)
        xyz, rgb, tri, (v, t) = HM.extract_mesh(vol.planes, vol.origin, vol.voxel, min_weight)
        assert (v, t) == (len(ref["xyz"]), len(ref["tri"]))
        MC.check_against(ref, xyz, rgb, tri, f"{name} at min_weight {min_weight}")
        # the vertices on the +x, +y, +z edges, in order, are the fusion library's surface points
        pts, cols = vol.extract(min_weight)
        axial = ref["e"] < 3
        assert MC.same_bits(xyz[axial], pts) and MC.same_bits(rgb[axial], cols), name
        triangles += t
    if FC.cases()[name]["calls"]:
        assert triangles > 100, name
    if name == "empty":
        assert triangles == 0


def test_planes_filled_by_hand_cover_every_case():
    ref = MC.direct_reference()
    cases = ref["cases"]
    assert (cases[:, 1:15].sum(axis=1) > 0).all(), "a tetrahedron without a triangle"
    assert (cases[:, 1:15].sum(axis=0) > 0).all(), "one of the fourteen cases does not occur"
    planes = MC.direct_planes()
    flat = planes[0].reshape(-1)
    a, e = ref["a"], ref["e"]
    step = np.array(MO.EDGES) @ np.array([1, 7, 35])
    with np.errstate(all="ignore"):
        frac = flat[a] / (flat[a] - flat[a + step[e]])
    assert (frac == 1).any() and np.isnan(ref["xyz"]).any()  # (a vertex at an edge's end, one on a NaN voxel's edge)
    for min_weight in (MC.DIRECT_MIN_WEIGHT, 1.0, 3.0):
        ref = MC.direct_reference(min_weight)
        MC.check_against(ref, *_mesh(planes, MC.DIRECT_ORIGIN, MC.DIRECT_VOXEL, min_weight), f"min_weight {min_weight}")


@pytest.mark.parametrize("dims", [(1, 6, 5), (6, 1, 5), (6, 5, 1), (1, 1, 7), (1, 1, 1)])
def test_a_volume_one_voxel_thick_has_vertices_and_no_triangle(dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(5)
    planes = np.zeros((5, nz, ny, nx), np.float32)
    planes[0] = rng.uniform(-1, 1, (nz, ny, nx))
    planes[1] = rng.integers(0, 3, (nz, ny, nx))
    planes[2:] = rng.uniform(0, 1, (3, nz, ny, nx))
    ref = MO.mesh(planes, (0.0, 0.5, -0.5), 0.25, 1.0)
    xyz, rgb, tri, (v, t) = HM.extract_mesh(planes, (0.0, 0.5, -0.5), 0.25, 1.0)
    assert t == 0 and tri.shape == (0, 3) and v == len(ref["xyz"]) and (v > 0 or sorted(dims)[1] == 1)
    MC.check_against(ref, xyz, rgb, tri, str(dims))


def test_an_all_zero_volume_is_empty():
    planes = np.zeros((5, 6, 5, 7), np.float32)
    xyz, rgb, tri, totals = HM.extract_mesh(planes, (0.0, 0.0, 0.0), 0.1, 1.0)
    assert totals == (0, 0) and xyz.shape == (0, 3) and rgb.shape == (0, 3) and tri.shape == (0, 3)


def test_nothing_is_written_at_or_past_the_capacity():
    MC.check_capacity(_mesh, np.nan, HM.BYTE_FILL, HM.BYTE_FILL)


def test_the_sphere_is_a_closed_oriented_manifold():
    ref = MC.sphere_reference()
    xyz, rgb, tri = _mesh(MC.sphere_planes(), (0.0, 0.0, 0.0), MC.SPHERE_VOXEL, 1.0)
    MC.check_against(ref, xyz, rgb, tri, "sphere")
    err, bound = MC.check_sphere(xyz, tri)
    print(f"sphere: {len(xyz)} vertices, {len(tri)} triangles, largest distance to the sphere {err:.3e} (bound {bound:.3e})")


def test_two_runs_give_equal_bytes():
    vol = _fused("straddle_F5")
    first = _mesh(vol.planes, vol.origin, vol.voxel, 1.0)
    second = _mesh(vol.planes, vol.origin, vol.voxel, 1.0)
    assert all(MC.same_bits(a, b) for a, b in zip(first, second)) and len(first[2]) > 100
