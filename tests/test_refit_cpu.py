"""Refit of a CPU scene (ceres_cpu_scene_refit / _f64, `./render --cpu A.obj --refit B.obj`): the scene
after its triangles moved, topology kept, every box recomputed (hierarchy_refitter.hpp:17-32).  No GPU
needed.

Every comparison is against a FRESH CpuScene that the existing constructor builds from the moved triangles
and a BVH refitted in numpy (tests/refit_common.py) -- never against the refitted scene itself: frames,
RGB8, hit records and the traversal counters (node_pairs / tri_tests pin the boxes, not just the picture)
must be identical, float and double, in both arithmetics."""
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

import refit_common as rc

CASES = [(n, f64, arith) for n in rc.SCENES for f64 in (False, True) for arith in (0, 1)]
IDS = ["%s-%s-%s" % (n, "f64" if d else "f32", "fma" if a else "exact") for n, d, a in CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def case(name, f64, arith):
    """The inputs and the fresh scene's answers of one case, computed once and shared."""
    from conftest import import_package
    pkg = import_package()
    mesh, bvh, moved, moved_bvh = rc.moved_scene_inputs(pkg, name, f64, arith)
    basis, sun, W, H, mode = rc.pose_of(pkg, name, f64, arith)
    fresh = pkg.CpuScene(moved, moved_bvh)
    try:
        ans = answers(pkg, fresh, moved, basis, sun, W, H, mode, f64, arith)
    finally:
        fresh.close()
    return dict(mesh=mesh, bvh=bvh, moved=moved, basis=basis, sun=sun, W=W, H=H, mode=mode, fresh=ans)


def answers(pkg, scene, mesh, basis, sun, W, H, mode, f64, arith):
    """render, trace (closest + occluded on the frame's camera rays plus their shadow rays) and shade of a
    CpuScene, as bytes and counters."""
    qmode = mode & (pkg.MODE_FMA | pkg.MODE_ROBUST)
    px, rgb, st = scene.render(basis, sun, W, H, mode=mode)
    rays = (pkg.camera_rays64 if f64 else pkg.camera_rays)(basis, W, H, arith)
    hits, _, _ = scene.trace(rays, mode=qmode)
    srays, _ = (pkg.shadow_rays64 if f64 else pkg.shadow_rays)(mesh, hits, sun)
    allrays = np.concatenate([rays, srays])
    hits, occ, tst = scene.trace(allrays, mode=qmode, closest=True, occluded=True)
    spx, srgb, shits, status, sst = scene.shade(rays, sun, mode=qmode, pixels=True, rgb8=True, hits=True, status=True)
    keys = ("rays", "hits", "node_pairs", "tri_tests")
    return dict(px=px, rgb=rgb, st={k: st[k] for k in keys + ("primary_rays", "shadow_rays")},
                hits=hits, occ=occ, tst={k: tst[k] for k in keys},
                spx=spx, srgb=srgb, shits=shits, status=status, sst={k: sst[k] for k in keys})


def assert_same(a, b):
    for k in ("px", "rgb", "hits", "occ", "spx", "srgb", "shits", "status"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("st", "tst", "sst"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("name,f64,arith", CASES, ids=IDS)
def test_refit_equals_fresh_scene(pkg, name, f64, arith):
    c = case(name, f64, arith)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        s.refit(c["moved"])
        got = answers(pkg, s, c["moved"], c["basis"], c["sun"], c["W"], c["H"], c["mode"], f64, arith)
    finally:
        s.close()
    assert_same(got, c["fresh"])


@pytest.mark.parametrize("name", rc.SCENES)
def test_deformation_is_strong_enough(pkg, name):
    """On the fresh deformed scene alone: the frame differs from the undeformed one, primary rays hit at
    least a tenth of the pixels, and where the undeformed scene shows lit and shadowed pixels (bunny,
    dupleaf; a lone triangle or a flat quad cannot shadow itself) the deformed one shows both too.  Part of
    the moved body lies outside the old root box, so a stale root box or cull rectangle would show."""
    c = case(name, False, 0)
    mesh, bvh = c["mesh"], c["bvh"]
    s = pkg.CpuScene(mesh, bvh)
    try:
        px0, _, _ = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        rays = pkg.camera_rays(c["basis"], c["W"], c["H"])
        _, _, _, status0, _ = s.shade(rays, c["sun"], status=True)
    finally:
        s.close()
    f = c["fresh"]
    assert not np.array_equal(bits(px0), bits(f["px"]))
    assert np.count_nonzero(f["status"]) * 10 >= f["status"].size
    if {1, 2} <= set(np.unique(status0)):
        assert {1, 2} <= set(np.unique(f["status"]))
    assert name not in ("bunny_orbit7_160x120", "dupleaf") or {1, 2} <= set(np.unique(status0))
    old_root = rc.node_fields(bvh.nodes)[0][0]
    new = rc.tri_boxes(c["moved"].tri)
    assert np.any(new[:, 0::2] < old_root[0::2]) or np.any(new[:, 1::2] > old_root[1::2])


@pytest.mark.parametrize("name,f64,arith", CASES, ids=IDS)
def test_refit_back_to_the_original_mesh(pkg, name, f64, arith):
    """Deformed, then refitted back: the frame is the fresh ORIGINAL scene's -- and, where the reference
    rendered a fixture of the config (float: all four scenes; double: quad and tri1, the only ones among
    tests/golden/f64), its PPM sha256: a refit is exact, and on the reference builder's trees every parent
    box already is the union of its children's, so the refitted-back boxes are the builder's."""
    c = case(name, f64, arith)
    build = "ref" if arith else "exact"
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    orig = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        s.refit(c["moved"])
        s.refit(c["mesh"])
        px, rgb, st = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        opx, orgb, ost = orig.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
        orig.close()
    assert np.array_equal(bits(px), bits(opx)) and np.array_equal(rgb, orgb)
    assert [st[k] for k in ("rays", "hits", "node_pairs", "tri_tests")] == [ost[k] for k in ("rays", "hits", "node_pairs", "tri_tests")]
    meta = None
    if not f64:
        meta = load_golden(name)[0]
    elif os.path.exists(os.path.join(GOLDEN, "f64", name + ".json")):
        meta = json.load(open(os.path.join(GOLDEN, "f64", name + ".json")))
    assert f64 or meta is not None
    if meta is not None:
        assert hashlib.sha256(pkg.ppm(c["W"], c["H"], rgb)).hexdigest() == meta["ppm_sha256"][build]
        assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"])


@pytest.mark.parametrize("f64", [False, True])
def test_refit_errors_leave_the_scene_untouched(pkg, f64):
    """A wrong triangle count or a float / double mismatch is CERES_EINVAL and the scene renders its old frame."""
    import ctypes
    c = case("quad", f64, 0)
    other = case("quad", not f64, 0)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        with pytest.raises(pkg.CeresError):
            s.refit(pkg.Mesh(c["moved"].tri[:-1], c["moved"].norm[:-1]))
        with pytest.raises(pkg.CeresError):
            s.refit(other["moved"])
        L = pkg.lib()
        m = other["moved"]
        if f64:
            rcode = L.ceres_cpu_scene_refit(s._h, pkg._p(m.tri, ctypes.c_float), len(m), pkg._p(m.norm, ctypes.c_float))
        else:
            rcode = L.ceres_cpu_scene_refit_f64(s._h, pkg._p(m.tri, ctypes.c_double), len(m), pkg._p(m.norm, ctypes.c_double))
        assert rcode == -1 and b"scene" in L.ceres_last_error()
        assert (L.ceres_cpu_scene_refit_f64 if f64 else L.ceres_cpu_scene_refit)(s._h, None, len(m), None) == -1
        after = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert before[2]["node_pairs"] == after[2]["node_pairs"]


def test_refit_keeps_normals_when_none_are_given(pkg):
    """norm == NULL keeps the scene's normals: the frame equals a fresh scene of the moved triangles with
    the OLD normals."""
    import ctypes
    c = case("dupleaf", False, 0)
    moved = c["moved"]
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    fresh = pkg.CpuScene(pkg.Mesh(moved.tri, c["mesh"].norm), pkg.Bvh(rc.refit_nodes(c["bvh"].nodes, c["bvh"].prim, moved.tri), c["bvh"].prim))
    try:
        assert pkg.lib().ceres_cpu_scene_refit(s._h, pkg._p(moved.tri, ctypes.c_float), len(moved), None) == 0
        a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        b = fresh.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
        fresh.close()
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert not np.array_equal(bits(a[0]), bits(c["fresh"]["px"]))       # and the normals do matter to the frame


def cli(pkg, args):
    return subprocess.run([pkg.CLI_PATH] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("name", ["quad", "dupleaf"])
def test_cli_cpu_refit_writes_the_fresh_scene_ppm(pkg, tmp_path, name, double):
    """./render --cpu A.obj --refit B.obj [--double] writes the PPM bytes of a fresh scene of B over A's
    refitted BVH.  B is the deformed mesh written by the test's own OBJ writer and read back by the
    library's loader, as the CLI reads it."""
    cfg = pkg.configs.CONFIGS[name]
    arith = pkg.ARITH_FMA                                                  # the CLI's default arithmetic
    mesh, bvh, _ = pkg.prepare(cfg, f64=double, arith=arith)
    b_obj = str(tmp_path / "b.obj")
    rc.write_obj(b_obj, rc.deform(pkg.prepare(cfg, arith=arith)[0]))
    moved = (pkg.load_obj_f64 if double else pkg.load_obj)(b_obj, arith)
    assert len(moved) == len(mesh)
    basis, sun, W, H, mode = rc.pose_of(pkg, name, double, arith)
    fresh = pkg.CpuScene(moved, pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim))
    try:
        _, rgb, st = fresh.render(basis, sun, W, H, mode=mode)
    finally:
        fresh.close()
    out = str(tmp_path / "out.ppm")
    r = cli(pkg, pkg.configs.cli_args(cfg) + ["--cpu", "--refit", b_obj, "--json", "-o", out] + (["--double"] if double else []))
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == pkg.ppm(W, H, rgb)
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            got.update(json.loads(line))
    assert (got["rays"], got["hits"], got["node_pairs"], got["tri_tests"]) == (st["rays"], st["hits"], st["node_pairs"], st["tri_tests"])
    assert "Refitting" in r.stdout


def test_cli_cpu_refit_with_rays(pkg, tmp_path):
    """--refit composes with --rays: the hits of the file's rays against the refitted scene."""
    name = "quad"
    cfg = pkg.configs.CONFIGS[name]
    arith = pkg.ARITH_FMA
    mesh, bvh, _ = pkg.prepare(cfg, arith=arith)
    b_obj = str(tmp_path / "b.obj")
    rc.write_obj(b_obj, rc.deform(mesh))
    moved = pkg.load_obj(b_obj, arith)
    basis, sun, W, H, mode = rc.pose_of(pkg, name, False, arith)
    rays = pkg.camera_rays(basis, W, H, arith)
    rays.tofile(str(tmp_path / "rays.bin"))
    fresh = pkg.CpuScene(moved, pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim))
    try:
        hits, _, _ = fresh.trace(rays, mode=pkg.MODE_FMA)
    finally:
        fresh.close()
    r = cli(pkg, [pkg.configs.obj_path(cfg), "--cpu", "--refit", b_obj, "--rays", str(tmp_path / "rays.bin"),
                  "--hits-out", str(tmp_path / "hits.bin")])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "hits.bin"), "rb").read() == hits.tobytes()
    assert np.count_nonzero(hits["prim"] >= 0) > 0


def test_cli_refit_rejects_another_face_count(pkg, tmp_path):
    cfg = pkg.configs.CONFIGS["quad"]
    r = cli(pkg, [pkg.configs.obj_path(cfg), "--cpu", "--refit", os.path.join(GOLDEN, "tri1.obj"), "--size", "8", "8",
                  "-o", str(tmp_path / "x.ppm")])
    assert r.returncode == 1 and "face count" in r.stderr and not os.path.exists(str(tmp_path / "x.ppm"))
    r = cli(pkg, ["--proc", "5", "--cpu", "--refit", os.path.join(GOLDEN, "tri1.obj")])
    assert r.returncode == 2
    r = cli(pkg, [pkg.configs.obj_path(cfg), "--cpu", "--refit"])
    assert r.returncode == 2
