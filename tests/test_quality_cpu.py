"""Upkeep of a CPU scene (ceres_cpu_scene_sah_cost / _rebuild / _update and their _f64 siblings, `./render
--cpu A.obj --refit B.obj --rebuild-above R`): the SAH cost of the scene's tree, a rebuild behind the same
handle and the call that refits and rebuilds only when the cost has grown.  No GPU needed.

Costs are compared with the numpy model of tests/quality_common.py on reference-layout nodes, within the
bound derived there; scenes with FRESH CpuScenes that the existing constructor builds from the moved
triangles and a BVH the existing builder (rebuild) or the numpy refit (refit) made."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import quality_common as qc
import refit_common as rc

CASES = [(n, f64) for n in rc.SCENES for f64 in (False, True)]
IDS = ["%s-%s" % (n, "f64" if d else "f32") for n, d in CASES]
BUNNY = "bunny_orbit7_160x120"
# rebuild: every scene in exact arithmetic, the bunny in the reference build's arithmetic too
REBUILD_CASES = [(n, f64, 0) for n, f64 in CASES] + [(BUNNY, False, 1), (BUNNY, True, 1)]
REBUILD_IDS = ["%s-%s-%s" % (n, "f64" if d else "f32", "fma" if a else "exact") for n, d, a in REBUILD_CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def answers(pkg, scene, c, f64, arith=0):
    """render, trace (closest + occluded on the frame's camera rays) and shade of a CpuScene."""
    qmode = c["mode"] & (pkg.MODE_FMA | pkg.MODE_ROBUST)
    px, rgb, st = scene.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    rays = (pkg.camera_rays64 if f64 else pkg.camera_rays)(c["basis"], c["W"], c["H"], arith)
    hits, occ, tst = scene.trace(rays, mode=qmode, closest=True, occluded=True)
    spx, srgb, shits, status, sst = scene.shade(rays, c["sun"], mode=qmode, pixels=True, rgb8=True, hits=True, status=True)
    keys = ("rays", "hits", "node_pairs", "tri_tests")
    return dict(px=px, rgb=rgb, st={k: st[k] for k in keys}, hits=hits, occ=occ, tst={k: tst[k] for k in keys},
                spx=spx, srgb=srgb, shits=shits, status=status, sst={k: sst[k] for k in keys})


def assert_same(a, b):
    for k in ("px", "rgb", "hits", "occ", "spx", "srgb", "shits", "status"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("st", "tst", "sst"):
        assert a[k] == b[k], k


@functools.lru_cache(maxsize=None)
def fresh(name, f64, arith, which):
    """The answers of a fresh CpuScene of the MOVE mesh over the refitted (`refit`) or the rebuilt
    (`rebuilt`) BVH, computed once and shared."""
    from conftest import import_package
    pkg = import_package()
    c = qc.inputs(name, f64, arith)
    s = pkg.CpuScene(c["moved"], c["moved_bvh"] if which == "refit" else c["rebuilt_bvh"])
    try:
        return answers(pkg, s, c, f64, arith)
    finally:
        s.close()


@pytest.mark.parametrize("name,f64", CASES, ids=IDS)
def test_cost_matches_the_model(pkg, name, f64):
    """sah_cost as built and after refit(MOVE) matches the model; two calls return equal bits; the query
    leaves the scene's frame alone."""
    c = qc.inputs(name, f64)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        built, again = s.sah_cost(), s.sah_cost()
        after = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        s.refit(c["moved"])
        refitted, refitted_again = s.sah_cost(), s.sah_cost()
    finally:
        s.close()
    qc.assert_cost(built, c["bvh"].nodes, "as built")
    qc.assert_cost(refitted, c["moved_bvh"].nodes, "after the refit")
    assert qc.dbits(built) == qc.dbits(again) and qc.dbits(refitted) == qc.dbits(refitted_again)
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert before[2]["node_pairs"] == after[2]["node_pairs"]
    if name == "tri1":
        assert built == 1.0 and refitted == 1.0                       # the root is a leaf of one triangle


@pytest.mark.parametrize("name,f64,arith", REBUILD_CASES, ids=REBUILD_IDS)
def test_rebuild_equals_a_fresh_scene(pkg, name, f64, arith):
    """After rebuild(moved): frame, rays / hits, traversal counters, trace and shade equal those of a fresh
    CpuScene(moved, build_bvh(moved)); the cost matches the model on that BVH."""
    c = qc.inputs(name, f64, arith)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        s.rebuild(c["moved"], arith=arith)
        got = answers(pkg, s, c, f64, arith)
        cost = s.sah_cost()
    finally:
        s.close()
    assert_same(got, fresh(name, f64, arith, "rebuilt"))
    qc.assert_cost(cost, c["rebuilt_bvh"].nodes, "rebuilt")


@pytest.mark.parametrize("f64", [False, True])
def test_rebuild_keeps_normals_when_none_are_given(pkg, f64):
    """norm == NULL keeps the scene's normals: the frame equals a fresh scene of the moved triangles with
    the OLD normals over the rebuilt BVH, and differs from the one with the moved normals."""
    c = qc.inputs("dupleaf", f64)
    moved = pkg.Mesh(c["moved"].tri, c["moved"].norm)
    moved.norm = None
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    old = pkg.CpuScene(pkg.Mesh(c["moved"].tri, c["mesh"].norm), c["rebuilt_bvh"])
    try:
        s.rebuild(moved)
        a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        b = old.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
        old.close()
    assert np.array_equal(bits(a[0]), bits(b[0]))
    assert not np.array_equal(bits(a[0]), bits(fresh("dupleaf", f64, 0, "rebuilt")["px"]))


def close(got, nodes):
    want = qc.model_cost(nodes)
    return abs(got - want) <= qc.tolerance(nodes) * want


@pytest.mark.parametrize("name,f64", CASES, ids=IDS)
def test_update_never_rebuilds_at_infinity(pkg, name, f64):
    """max_ratio = +inf: a refit plus a measurement -- rebuilt == 0, the answers are the fresh scene's over
    the refitted BVH, the info fields match the model."""
    c = qc.inputs(name, f64)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        u = s.update(c["moved"], math.inf)
        got = answers(pkg, s, c, f64)
    finally:
        s.close()
    print(u)
    assert u["rebuilt"] == 0
    assert close(u["built_cost"], c["bvh"].nodes) and close(u["cost"], c["moved_bvh"].nodes)
    assert qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
    assert_same(got, fresh(name, f64, 0, "refit"))


@pytest.mark.parametrize("name,f64", CASES, ids=IDS)
def test_update_rebuilds_below_the_ratio(pkg, name, f64):
    """max_ratio = 0.9 r (r: the model's ratio of the case): rebuilt == 1, the answers are the fresh rebuilt
    scene's; a second update with OTHER reports the rebuilt tree's cost as its baseline."""
    c = qc.inputs(name, f64)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        u = s.update(c["moved"], 0.9 * c["r"])
        got = answers(pkg, s, c, f64)
        v = s.update(c["other"], math.inf)
    finally:
        s.close()
    print(u, v)
    assert u["rebuilt"] == 1
    assert close(u["built_cost"], c["bvh"].nodes) and close(u["cost"], c["moved_bvh"].nodes)
    assert close(u["new_cost"], c["rebuilt_bvh"].nodes)
    assert_same(got, fresh(name, f64, 0, "rebuilt"))
    assert v["rebuilt"] == 0 and qc.dbits(v["built_cost"]) == qc.dbits(u["new_cost"])
    assert close(v["cost"], c["other_bvh"].nodes)


@pytest.mark.parametrize("name,f64", CASES, ids=IDS)
def test_update_keeps_the_tree_above_the_ratio(pkg, name, f64):
    """max_ratio = 1.1 r keeps the tree: rebuilt == 0 and the frame with its traversal counters is the
    refitted scene's."""
    c = qc.inputs(name, f64)
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        u = s.update(c["moved"], 1.1 * c["r"])
        px, rgb, st = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
    f = fresh(name, f64, 0, "refit")
    assert u["rebuilt"] == 0 and close(u["cost"], c["moved_bvh"].nodes) and qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
    assert np.array_equal(bits(px), bits(f["px"])) and {k: st[k] for k in f["st"]} == f["st"]


@pytest.mark.parametrize("f64", [False, True])
def test_errors_leave_the_scene_untouched(pkg, f64):
    """A wrong triangle count, a float / double mismatch, null pointers, max_ratio NaN / 0 / negative and a
    bad arith are CERES_EINVAL, and the scene renders its old frame."""
    c = qc.inputs("quad", f64)
    o = qc.inputs("quad", not f64)
    L = pkg.lib()
    ct, oct_ = (ctypes.c_double, ctypes.c_float) if f64 else (ctypes.c_float, ctypes.c_double)
    rebuild, update = (L.ceres_cpu_scene_rebuild_f64, L.ceres_cpu_scene_update_f64) if f64 else (L.ceres_cpu_scene_rebuild, L.ceres_cpu_scene_update)
    wrong_rebuild, wrong_update = (L.ceres_cpu_scene_rebuild, L.ceres_cpu_scene_update) if f64 else (L.ceres_cpu_scene_rebuild_f64, L.ceres_cpu_scene_update_f64)
    m, om = c["moved"], o["moved"]
    tri, norm, n = pkg._p(m.tri, ct), pkg._p(m.norm, ct), len(m)
    info = pkg._UpdateInfo()
    s = pkg.CpuScene(c["mesh"], c["bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        short = pkg.Mesh(m.tri[:-1], m.norm[:-1])
        for call in (lambda: s.rebuild(short), lambda: s.update(short, 2.0), lambda: s.rebuild(om), lambda: s.update(om, 2.0)):
            with pytest.raises(pkg.CeresError):
                call()
        codes = [
            rebuild(s._h, tri, n - 1, norm, 0), update(s._h, tri, n + 1, norm, 0, 2.0, None),
            wrong_rebuild(s._h, pkg._p(om.tri, oct_), n, pkg._p(om.norm, oct_), 0),
            wrong_update(s._h, pkg._p(om.tri, oct_), n, pkg._p(om.norm, oct_), 0, 2.0, ctypes.byref(info)),
            rebuild(s._h, None, n, None, 0), update(s._h, None, n, None, 0, 2.0, None),
            rebuild(None, tri, n, norm, 0), update(None, tri, n, norm, 0, 2.0, None),
            update(s._h, tri, n, norm, 0, math.nan, None), update(s._h, tri, n, norm, 0, 0.0, None),
            update(s._h, tri, n, norm, 0, -1.0, ctypes.byref(info)),
            rebuild(s._h, tri, n, norm, 7), update(s._h, tri, n, norm, -1, 2.0, None),
            L.ceres_cpu_scene_sah_cost(None, ctypes.byref(ctypes.c_double())), L.ceres_cpu_scene_sah_cost(s._h, None),
        ]
        after = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        cost = s.sah_cost()
    finally:
        s.close()
    assert codes == [-1] * len(codes), codes
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert before[2]["node_pairs"] == after[2]["node_pairs"]
    qc.assert_cost(cost, c["bvh"].nodes, "after the refusals")


def cli(pkg, args):
    return subprocess.run([pkg.CLI_PATH] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("double", [False, True])
def test_cli_cpu_rebuild_above(pkg, tmp_path, double):
    """./render --cpu A.obj --refit B.obj --rebuild-above 1e-9 writes the PPM of ./render --cpu B.obj (the
    tree is rebuilt for B); --rebuild-above 1e30 writes the PPM of plain --refit (the tree is kept); one
    line reports the cost, the baseline, the ratio and what was done; the flag without --refit is bad usage."""
    cfg = pkg.configs.CONFIGS["dupleaf"]
    a_args = pkg.configs.cli_args(cfg) + ["--cpu"] + (["--double"] if double else [])
    b_obj = str(tmp_path / "b.obj")
    rc.write_obj(b_obj, rc.deform(pkg.prepare(cfg, arith=pkg.ARITH_FMA)[0]))
    b_args = [b_obj if x == pkg.configs.obj_path(cfg) else x for x in a_args]
    assert b_args != a_args
    out = {k: str(tmp_path / (k + ".ppm")) for k in ("b", "refit", "low", "high")}
    runs = {"b": cli(pkg, b_args + ["-o", out["b"]]),
            "refit": cli(pkg, a_args + ["--refit", b_obj, "-o", out["refit"]]),
            "low": cli(pkg, a_args + ["--refit", b_obj, "--rebuild-above", "1e-9", "-o", out["low"]]),
            "high": cli(pkg, a_args + ["--refit", b_obj, "--rebuild-above", "1e30", "-o", out["high"]])}
    for k, r in runs.items():
        assert r.returncode == 0, (k, r.stderr)
    ppm = {k: open(p, "rb").read() for k, p in out.items()}
    assert ppm["low"] == ppm["b"] and ppm["high"] == ppm["refit"]
    low = [ln for ln in runs["low"].stdout.splitlines() if ln.startswith("SAH cost")]
    high = [ln for ln in runs["high"].stdout.splitlines() if ln.startswith("SAH cost")]
    assert len(low) == 1 and low[0].endswith("rebuilt") and len(high) == 1 and high[0].endswith("kept")
    assert "built:" in low[0] and "ratio:" in low[0]
    r = cli(pkg, a_args + ["--rebuild-above", "1.2", "-o", str(tmp_path / "x.ppm")])
    assert r.returncode == 2 and not os.path.exists(str(tmp_path / "x.ppm"))
