"""Closest-point queries on double scenes on host cores (ceres_closest_points_cpu_f64; CpuScene.closest_points_f64)
against the float64 brute force of closest64_common.py -- byte for byte, because the contract makes the answer
the minimum over all triangles of one float64 formula, whatever the tree."""
import ctypes

import numpy as np
import pytest

import closest64_common as c64
import closest_common as cc
import deep_common as dc

EINVAL, EUNSUPPORTED = -1, -6
CAP26_DEPTH = 64                                                      # Scene.info()["depth"] of the double cap26 tree


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("closest64")


@pytest.mark.parametrize("name", c64.SCENES)
def test_cpu_equals_the_model(pkg, tmp, name):
    """Every scene, every set, at threads 1, 0 and 3: the model's bytes."""
    mesh, bvh = c64.scene(name, tmp)
    assert mesh.f64
    sets, near = c64.expected(name, tmp)
    pts, want = c64.joined(sets), c64.joined(near)
    sc = pkg.CpuScene(mesh, bvh)
    for threads in (1, 0, 3):
        got, st = sc.closest_points_f64(pts, threads=threads)
        assert got.dtype == pkg.NEAR64_DTYPE
        assert c64.same(got, want), c64.first_difference(got, want, pts)
        assert st["rays"] == len(pts) and st["hits"] == int((want["prim"] >= 0).sum())
        assert st["tri_tests"] >= st["hits"]
    got3, _ = sc.closest_points_f64(sets["a_uniform"][:, :3])             # [n, 3] points mean r2max = +inf
    assert c64.same(got3, near["a_uniform"])
    sc.close()
    if name == "cap26":                                                   # the deepest legal stack of the GPU walk
        assert dc.depth_and_leaf(bvh.nodes)[0] == CAP26_DEPTH


def test_the_sets_exercise_what_they_are_for():
    """Exact multi-way ties on the mesh points, both outcomes of every finite radius, misses for NaN -- in double."""
    mesh, _ = c64.scene("bunny")
    sets, near = c64.expected("bunny")
    d2 = cc.pair_d2(mesh.tri, sets["b_on_mesh"], np.float64)[0]
    ties = (d2 == near["b_on_mesh"]["d2"][:, None]).sum(axis=1)
    assert (ties >= 2).sum() >= len(ties) // 2 and ties.max() >= 5, ties
    e, r = near["e_radius"], sets["e_radius"][:, 3]
    assert (e["prim"][1::5] >= 0).all() and (e["d2"][1::5] == r[1::5]).all()          # a surface at exactly r2max counts
    assert (e["prim"][2::5] == -1).all() and (e["prim"][3::5] == -1).all() and (e["prim"][4::5] == -1).all()
    assert (e["prim"][0::5] >= 0).any() and (e["prim"][0::5] == -1).any()             # r2max = 0: on the mesh or not
    assert (r[2::5] == -5e-324).any() and (r[2::5] > 0).any()                         # below a best of 0, below a positive best
    f = near["f_nonfinite"]
    nan = np.isnan(sets["f_nonfinite"][:, :3]).any(axis=1)
    assert (f["prim"][nan] == -1).all()
    all_near = c64.joined(near)
    miss = all_near["prim"] < 0
    assert miss.any() and (all_near.view(np.uint64).reshape(-1, 4)[miss] == [0xffffffff, 0, 0, 0]).all()
    assert (all_near["pad"] == 0).all()
    # the double answers are not the float ones widened: the float model of the same points differs in d2
    f32 = cc.model32(mesh.tri.astype(np.float32), sets["a_uniform"].astype(np.float32))
    assert (f32["d2"].astype(np.float64) != near["a_uniform"]["d2"]).any()


def test_a_nan_d2_is_never_taken(pkg):
    """Finite triangles so large that their d2 is NaN (closest64_common.overflow_mesh, size 1e200) are skipped."""
    mesh = c64.overflow_mesh(pkg)
    sets = c64.base_sets(mesh.tri[0::2])
    pts = np.concatenate([sets[k] for k in c64.ORDER[:4]])
    d2 = cc.pair_d2(mesh.tri, pts, np.float64)[0]
    assert np.isnan(d2[:, 1::2]).any() and not np.isnan(d2[:, 0::2]).any()
    want = c64.model64_exact(mesh.tri, pts)
    assert (want["prim"] >= 0).all()
    sc = pkg.CpuScene(mesh, pkg.build_bvh(mesh))
    got, _ = sc.closest_points_f64(pts)
    sc.close()
    assert c64.same(got, want), c64.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["quad", "bunny", "arms6", "bodyarms"])
def test_the_answer_does_not_depend_on_the_tree(pkg, name):
    """The reference-order BVH, the same scene rebuilt in another arithmetic, and refit, rebuild and update to a
    moved mesh (against the model on the moved mesh): the same bytes."""
    mesh, bvh = c64.scene(name)
    sets, near = c64.expected(name)
    pts, want = c64.joined(sets), c64.joined(near)
    sc = pkg.CpuScene(mesh, bvh)
    sc.rebuild(mesh, pkg.ARITH_FMA)
    got, _ = sc.closest_points_f64(pts)
    assert c64.same(got, want), c64.first_difference(got, want, pts)
    moved = c64.moved_mesh(pkg, mesh, name)
    want_moved = c64.model64_exact(moved.tri, pts)
    assert not c64.same(want_moved, want)
    sc.refit(moved)
    got, _ = sc.closest_points_f64(pts)
    assert c64.same(got, want_moved), c64.first_difference(got, want_moved, pts)
    sc.rebuild(moved)
    got, _ = sc.closest_points_f64(pts)
    assert c64.same(got, want_moved), c64.first_difference(got, want_moved, pts)
    sc.close()
    sc = pkg.CpuScene(mesh, bvh)
    assert sc.update(moved, 1e-9)["rebuilt"] == 1
    got, _ = sc.closest_points_f64(pts)
    assert c64.same(got, want_moved), c64.first_difference(got, want_moved, pts)
    sc.close()


def _finite_points(sets):
    return np.concatenate([sets[k] for k in c64.ORDER[:4]])


def test_accuracy_against_longdouble(pkg):
    """|d2 - d2_long| / (eps M (sqrt(d2_long) + eps M)), eps = 2^-53, M = max|point| + max|vertex|, over the
    finite sets (a) .. (d) of bunny, quad, arms6, bodyarms and bunny_far (the double bunny with every p0 and
    every point translated by (2^27, -2^26, 2^25)); d2_long is (1) the np.longdouble distance to the winning
    triangle and (2) the np.longdouble minimum over all triangles.  The bound is four times the largest figure
    the float64 MODEL gives on these sets -- a margin for rounding differences between inputs, not
    implementation slack; the library returns the model's bytes (test_cpu_equals_the_model).
    Measured maxima (the model's and the library's alike; printed with -s): bunny 2.06, quad 1.67, arms6 1.18,
    bodyarms 1.87, bunny_far 1.65, the same against the winning triangle and against the long-double minimum;
    bounds 8.2, 6.7, 4.7, 7.5 and 6.6.  On bunny_far's inputs rounded to float the float path stands at
    5.3e8 of these units (a figure, not an assertion): float has run out there, double has not."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is no wider than double here")
    worst = {}
    for name in ("bunny", "quad", "arms6", "bodyarms", "bunny_far"):
        if name == "bunny_far":
            mesh0, _ = c64.scene("bunny")
            mesh = c64.far_mesh(pkg, mesh0)
            pts = _finite_points(c64.expected("bunny")[0]).copy()
            pts[:, :3] += c64.FAR
            bvh = pkg.build_bvh(mesh)
            model = c64.model64_exact(mesh.tri, pts)
        else:
            mesh, bvh = c64.scene(name)
            sets, near = c64.expected(name)
            pts = _finite_points(sets)
            model = np.concatenate([near[k] for k in c64.ORDER[:4]])
        assert (model["prim"] >= 0).all()
        lo, own = c64.model_long(mesh.tri, pts, model["prim"])
        bound = 4 * max(c64.error_units(model["d2"], own, mesh.tri, pts).max(), c64.error_units(model["d2"], lo, mesh.tri, pts).max())
        sc = pkg.CpuScene(mesh, bvh)
        got, _ = sc.closest_points_f64(pts)
        sc.close()
        _, own_got = c64.model_long(mesh.tri, pts, got["prim"])
        e_own = c64.error_units(got["d2"], own_got, mesh.tri, pts).max()
        e_min = c64.error_units(got["d2"], lo, mesh.tri, pts).max()
        worst[name] = (float(e_own), float(e_min), float(bound))
        print("closest-point error units (eps 2^-53) %s: winner %.3f, long-double minimum %.3f, bound %.3f" % (name, e_own, e_min, bound))
        assert e_own < bound and e_min < bound, worst
        assert bound < 32, worst                                      # the formula's own error stays a few units
        if name == "bunny_far":                                       # the float path on the same inputs: a figure only
            m32 = pkg.Mesh(mesh.tri.astype(np.float32), mesh.norm.astype(np.float32))
            s32 = pkg.CpuScene(m32, pkg.build_bvh(m32))
            g32, _ = s32.closest_points(pts.astype(np.float32))
            s32.close()
            hit = g32["prim"] >= 0
            e32 = c64.error_units(g32["d2"][hit], lo[hit], mesh.tri, pts).max()
            print("closest-point error units (eps 2^-53) bunny_far, the FLOAT path on the inputs rounded to float: %.3g" % e32)


def test_refusals(pkg):
    L = pkg.lib()
    mesh, bvh = c64.scene("quad")
    sc = pkg.CpuScene(mesh, bvh)
    pts = np.ascontiguousarray(c64.expected("quad")[0]["a_uniform"])
    out = np.full(len(pts) * 8 + 8, 0x5a5a5a5a, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    call = L.ceres_closest_points_cpu_f64
    assert call(None, vp(pts), len(pts), vp(out), None, 0) == EINVAL
    assert b"null scene" in L.ceres_last_error()
    assert call(sc._h, None, len(pts), vp(out), None, 0) == EINVAL
    assert call(sc._h, vp(pts), len(pts), None, None, 0) == EINVAL
    assert call(sc._h, vp(pts), 1 << 31, vp(out), None, 0) == EUNSUPPORTED
    assert (out == 0x5a5a5a5a).all()
    assert call(sc._h, vp(pts), 0, vp(out), None, 0) == 0                 # n_points = 0 writes nothing
    assert call(sc._h, None, 0, vp(out), None, 0) == 0
    assert (out == 0x5a5a5a5a).all()
    assert call(sc._h, vp(pts), len(pts), vp(out), None, 0) == 0
    assert out[-8:].tolist() == [0x5a5a5a5a] * 8 and not (out[:-8] == 0x5a5a5a5a).all()
    sc.close()
    mesh32, bvh32 = cc.scene("quad")                                      # a float scene handed to the _f64 call
    sc32 = pkg.CpuScene(mesh32, bvh32)
    out[:] = 0x5a5a5a5a
    assert call(sc32._h, vp(pts), len(pts), vp(out), None, 0) == EUNSUPPORTED
    assert b"_f64 closest-point calls take double scenes" in L.ceres_last_error()
    assert (out == 0x5a5a5a5a).all()
    with pytest.raises(pkg.CeresError, match="double scenes"):
        sc32.closest_points_f64(pts)
    sc32.close()
    with pytest.raises(pkg.CeresError, match="float64"):
        pkg._points32(np.zeros((3, 5)))


def test_abi_and_kernel_names(pkg):
    L = pkg.lib()
    for sym in ("ceres_closest_points_f64", "ceres_closest_points_f64_device", "ceres_closest_points_f64_indexed_device",
                "ceres_closest_points_cpu_f64"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    names = L.ceres_kernel_names().decode().split(",")
    assert "ceres_closest_points64_k" in names and "ceres_closest_points64_idx_k" in names
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"ceres_closest_points64_k" in blob and b"ceres_closest_points64_idx_k" in blob
    assert " 0.8 " in L.ceres_version().decode()
    assert pkg.NEAR64_DTYPE == c64.NEAR64_DTYPE and pkg.NEAR64_DTYPE.itemsize == 32
