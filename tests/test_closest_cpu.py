"""Closest-point queries on host cores (ceres_closest_points_cpu; CpuScene.closest_points; `./render --cpu
--points --nearest-out`), against the numpy brute force of closest_common.py -- byte for byte, because the
contract makes the answer the minimum over all triangles of one float32 formula, whatever the tree."""
import ctypes
import subprocess

import numpy as np
import pytest

import closest_common as cc

EINVAL, EUNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("closest")


@pytest.mark.parametrize("name", cc.SCENES)
def test_cpu_equals_the_model(pkg, tmp, name):
    """Every scene, every set, at threads 1 and 0: the model's bytes."""
    mesh, bvh = cc.scene(name, tmp)
    sets, near = cc.expected(name, tmp)
    pts, want = cc.joined(sets), cc.joined(near)
    sc = pkg.CpuScene(mesh, bvh)
    for threads in (1, 0):
        got, st = sc.closest_points(pts, threads=threads)
        assert cc.same(got, want), cc.first_difference(got, want, pts)
        assert st["rays"] == len(pts) and st["hits"] == int((want["prim"] >= 0).sum())
        assert st["tri_tests"] >= st["hits"]
    # [n, 3] points mean r2max = +inf
    got3, _ = sc.closest_points(sets["a_uniform"][:, :3])
    assert cc.same(got3, near["a_uniform"])
    sc.close()


def test_the_sets_exercise_what_they_are_for(tmp):
    """Exact multi-way ties on the mesh points, both outcomes of every finite radius, misses for NaN."""
    mesh, _ = cc.scene("bunny")
    sets, near = cc.expected("bunny")
    d2 = cc.pair_d2(mesh.tri, sets["b_on_mesh"])[0]
    ties = (d2 == near["b_on_mesh"]["d2"][:, None]).sum(axis=1)
    assert (ties >= 2).sum() >= len(ties) // 2 and ties.max() >= 5, ties
    e, r = near["e_radius"], sets["e_radius"][:, 3]
    assert (e["prim"][1::5] >= 0).all() and (e["d2"][1::5] == r[1::5]).all()          # a surface at exactly r2max counts
    assert (e["prim"][2::5] == -1).all() and (e["prim"][3::5] == -1).all() and (e["prim"][4::5] == -1).all()
    assert (e["prim"][0::5] >= 0).any() and (e["prim"][0::5] == -1).any()             # r2max = 0: on the mesh or not
    f = near["f_nonfinite"]
    nan = np.isnan(sets["f_nonfinite"][:, :3]).any(axis=1)
    assert (f["prim"][nan] == -1).all()
    miss = cc.joined(near)["prim"] < 0
    assert (cc.joined(near).view(np.uint32).reshape(-1, 4)[miss] == [0xffffffff, 0, 0, 0]).all()
    # dupleaf: coincident triangles, the smallest index wins
    dmesh, _ = cc.scene("dupleaf")
    dsets, dnear = cc.expected("dupleaf")
    dd = cc.pair_d2(dmesh.tri, dsets["a_uniform"])[0]
    win = dnear["a_uniform"]["prim"]
    tied = dd == dnear["a_uniform"]["d2"][:, None]
    assert (tied.sum(axis=1) >= 2).any() and (win == tied.argmax(axis=1)).all()
    assert not np.isnan(cc.joined(cc.expected("degenerate")[1])["d2"]).any()


def test_a_nan_d2_is_never_taken(pkg):
    """Finite triangles so large that their d2 is NaN (closest_common.overflow_mesh) are skipped: the answer
    is the minimum over the others."""
    mesh = cc.overflow_mesh(pkg)
    sets = cc.base_sets(mesh.tri[0::2])
    pts = np.concatenate([sets[k] for k in cc.ORDER[:4]])
    d2 = cc.pair_d2(mesh.tri, pts)[0]
    assert np.isnan(d2[:, 1::2]).any() and not np.isnan(d2[:, 0::2]).any()
    want = cc.model32(mesh.tri, pts)
    assert (want["prim"] >= 0).all()
    sc = pkg.CpuScene(mesh, pkg.build_bvh(mesh))
    got, _ = sc.closest_points(pts)
    sc.close()
    assert cc.same(got, want), cc.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["quad", "bunny", "arms6", "bodyarms"])
def test_the_answer_does_not_depend_on_the_tree(pkg, name):
    """The reference-order BVH, the same scene rebuilt, and a refit to a moved mesh (against the model on the
    moved mesh): the same bytes -- the independence claim."""
    mesh, bvh = cc.scene(name)
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    sc = pkg.CpuScene(mesh, bvh)
    sc.rebuild(mesh, pkg.ARITH_FMA)                                   # another arithmetic: another tree where it differs
    got, _ = sc.closest_points(pts)
    assert cc.same(got, want), cc.first_difference(got, want, pts)
    moved = cc.moved_mesh(pkg, mesh, name)
    want_moved = cc.model32(moved.tri, pts)
    assert not cc.same(want_moved, want)
    sc.refit(moved)
    got, _ = sc.closest_points(pts)
    assert cc.same(got, want_moved), cc.first_difference(got, want_moved, pts)
    sc.rebuild(moved)
    got, _ = sc.closest_points(pts)
    assert cc.same(got, want_moved), cc.first_difference(got, want_moved, pts)
    sc.close()


def test_accuracy_against_float64(pkg):
    """|d2_32 - d2_64| / (eps M (sqrt(d2_64) + eps M)), eps = 2^-24, M = max|point| + max|vertex|, over the
    finite sets (a) .. (d) of bunny, quad, arms6 and bodyarms; d2_64 is (1) the double distance to the winning
    triangle and (2) the double minimum over all triangles (near-ties may pick another triangle: distances are
    compared, not indices).  The bound is four times the largest figure the float32 MODEL gives on these sets
    -- a margin for rounding differences between inputs, not implementation slack; the library's answers are
    the model's bytes (test_cpu_equals_the_model), so they sit at a quarter of it.
    Measured maxima (the model's and the library's alike; printed with -s): bunny 2.52, quad 1.39, arms6 1.89,
    bodyarms 2.95, the same against the winning triangle and against the double minimum; bounds 10.1, 5.6, 7.6
    and 11.8."""
    worst = {}
    for name in ("bunny", "quad", "arms6", "bodyarms"):
        mesh, bvh = cc.scene(name)
        sets, near = cc.expected(name)
        keys = cc.ORDER[:4]
        pts = np.concatenate([sets[k] for k in keys])
        model = np.concatenate([near[k] for k in keys])
        assert (model["prim"] >= 0).all()
        lo, own = cc.model64(mesh.tri, pts, model["prim"])
        bound = 4 * max(cc.error_units(model["d2"], own, mesh.tri, pts).max(), cc.error_units(model["d2"], lo, mesh.tri, pts).max())
        sc = pkg.CpuScene(mesh, bvh)
        got, _ = sc.closest_points(pts)
        sc.close()
        _, own_got = cc.model64(mesh.tri, pts, got["prim"])
        e_own = cc.error_units(got["d2"], own_got, mesh.tri, pts).max()
        e_min = cc.error_units(got["d2"], lo, mesh.tri, pts).max()
        worst[name] = (float(e_own), float(e_min), float(bound))
        print("closest-point error units %s: winner %.3f, double minimum %.3f, bound %.3f" % (name, e_own, e_min, bound))
        assert e_own < bound and e_min < bound, worst
        assert bound < 4 * 8, worst                                   # the formula's own error stays a few units


def test_refusals(pkg):
    L = pkg.lib()
    mesh, bvh = cc.scene("quad")
    sc = pkg.CpuScene(mesh, bvh)
    pts = np.ascontiguousarray(cc.expected("quad")[0]["a_uniform"])
    out = np.full(len(pts) * 4 + 4, 0x5a5a5a5a, np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    assert L.ceres_closest_points_cpu(None, vp(pts), len(pts), vp(out), None, 0) == EINVAL
    assert b"null scene" in L.ceres_last_error()
    assert L.ceres_closest_points_cpu(sc._h, None, len(pts), vp(out), None, 0) == EINVAL
    assert L.ceres_closest_points_cpu(sc._h, vp(pts), len(pts), None, None, 0) == EINVAL
    assert L.ceres_closest_points_cpu(sc._h, vp(pts), 1 << 31, vp(out), None, 0) == EUNSUPPORTED
    assert (out == 0x5a5a5a5a).all()
    assert L.ceres_closest_points_cpu(sc._h, vp(pts), 0, vp(out), None, 0) == 0       # n_points = 0 writes nothing
    assert L.ceres_closest_points_cpu(sc._h, None, 0, vp(out), None, 0) == 0
    assert (out == 0x5a5a5a5a).all()
    assert L.ceres_closest_points_cpu(sc._h, vp(pts), len(pts), vp(out), None, 0) == 0
    assert out[-4:].tolist() == [0x5a5a5a5a] * 4 and not (out[:-4] == 0x5a5a5a5a).all()
    sc.close()
    mesh64, bvh64, _ = pkg.prepare(pkg.configs.CONFIGS["quad"], f64=True)
    sc64 = pkg.CpuScene(mesh64, bvh64)
    out[:] = 0x5a5a5a5a
    assert L.ceres_closest_points_cpu(sc64._h, vp(pts), len(pts), vp(out), None, 0) == EUNSUPPORTED
    assert b"closest-point queries take float scenes" in L.ceres_last_error()
    assert (out == 0x5a5a5a5a).all()
    with pytest.raises(pkg.CeresError, match="float scenes"):
        sc64.closest_points(pts)
    sc64.close()
    with pytest.raises(pkg.CeresError, match="points"):
        pkg._points16(np.zeros((3, 5), np.float32))


def test_abi_and_kernel_names(pkg):
    L = pkg.lib()
    for sym in ("ceres_closest_points", "ceres_closest_points_device", "ceres_closest_points_indexed_device",
                "ceres_closest_points_cpu"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    names = L.ceres_kernel_names().decode().split(",")
    assert "ceres_closest_points_k" in names and "ceres_closest_points_idx_k" in names
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"ceres_closest_points_k" in blob and b"ceres_closest_points_idx_k" in blob
    assert " 0.8 " in L.ceres_version().decode()
    assert pkg.NEAR_DTYPE == cc.NEAR_DTYPE and pkg.NEAR_DTYPE.itemsize == 16


def test_cli_cpu_writes_the_library_bytes(pkg, tmp):
    mesh, bvh = cc.scene("bunny")
    sets, near = cc.expected("bunny")
    pts, want = cc.joined(sets), cc.joined(near)
    obj = pkg.configs.obj_path(pkg.configs.CONFIGS[cc.CONFIG["bunny"]])
    pfile, ofile = cc.write_points(tmp / "p.bin", pts), str(tmp / "near.bin")
    cfg = pkg.configs.CONFIGS[cc.CONFIG["bunny"]]
    rot = ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    r = subprocess.run([pkg.CLI_PATH, obj, *rot, "--exact", "--cpu", "--threads", "2", "--points", pfile, "--nearest-out", ofile, "--json"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert '"points": %d' % len(pts) in r.stdout
    sc = pkg.CpuScene(mesh, bvh)
    got, _ = sc.closest_points(pts)
    sc.close()
    assert open(ofile, "rb").read() == got.tobytes() == want.tobytes()
    # --double: the library's refusal, status 1
    r = subprocess.run([pkg.CLI_PATH, obj, "--cpu", "--double", "--points", pfile, "--nearest-out", ofile], capture_output=True, text=True)
    assert r.returncode == 1 and "closest-point queries take float scenes" in r.stderr


def test_cli_usage_errors(pkg, tmp):
    obj = pkg.configs.obj_path(pkg.configs.CONFIGS["quad"])
    pfile = cc.write_points(tmp / "q.bin", cc.expected("quad")[0]["a_uniform"])
    out = str(tmp / "unused.bin")
    for args in (["--points", pfile],                                                  # no --nearest-out
                 ["--nearest-out", out],                                               # no --points
                 ["--points", pfile, "--nearest-out", out, "--rays", pfile, "--hits-out", out],
                 ["--points", pfile, "--nearest-out", out, "--hits-out", out],
                 ["--points"]):
        r = subprocess.run([pkg.CLI_PATH, obj, "--cpu"] + args, capture_output=True, text=True)
        assert r.returncode == 2, (args, r.stderr)
    odd = tmp / "odd.bin"
    odd.write_bytes(b"\0" * 24)
    r = subprocess.run([pkg.CLI_PATH, obj, "--cpu", "--points", str(odd), "--nearest-out", out], capture_output=True, text=True)
    assert r.returncode == 2 and "16-byte point records" in r.stderr
