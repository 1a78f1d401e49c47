"""Scenes with BVHs of 40 to 64 levels on the host (tests/deep_common.py; no GPU needed): the meshes
reach the regimes they are there for, the views are not trivial, and the host builder, the CPU
path, the entry cut and the scene upkeep agree with the reference on them.  Every comparison is
bitwise.  The frames of the arms6_* / bodyarms_* configs are held to their fixtures by the suites
parametrised over the fixtures (test_cpu_path.py, test_host_scene.py, test_oracle_golden.py, the
ray sets of test_trace_cpu.py); this file adds what those do not ask and everything about cap26,
which is no config."""
import functools
import hashlib
import math

import numpy as np
import pytest

from conftest import import_package, load_golden, load_ref_records

import configs
import deep_common as dc
import entry_common as E
import quality_common as qc
import refit_common as rc
from test_gpu_shadow_stack import _bounds

ARITHS = [0, 1]
BUILD = {0: "exact", 1: "ref"}


@pytest.fixture(scope="module")
def cap26_obj(tmp_path_factory):
    return dc.obj_path("cap26", tmp_path_factory.mktemp("cap26"))


@functools.lru_cache(maxsize=None)
def _load(path, arith):
    pkg = import_package()
    mesh = pkg.load_obj(path, arith)
    return mesh, pkg.build_bvh(mesh, arith)


def scene_of(name, arith, cap26_obj):
    return _load(cap26_obj if name == "cap26" else dc.obj_path(name), arith)


@pytest.mark.parametrize("name", ["arms6", "bodyarms"])
def test_obj_is_the_generators(name):
    with open(dc.obj_path(name), "rb") as f:
        assert f.read() == dc.obj_text(dc.MESHES[name]())


def test_cap26_is_its_fixtures_mesh(cap26_obj):
    with open(cap26_obj, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == dc.CAP26_SHA256 == dc.load_cap26()["obj_sha256"]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(dc.MESHES))
def test_regimes(pkg, name, arith, cap26_obj):
    """The conditions each mesh exists for, in both arithmetics (the values: DESIGN.md "Deep trees")."""
    mesh, bvh = scene_of(name, arith, cap26_obj)
    assert np.isfinite(mesh.tri).all() and np.isfinite(mesh.norm).all()
    depth, leaf = dc.depth_and_leaf(bvh.nodes)
    near, first = _bounds(bvh.nodes)                                  # asserts: no leaf above 31 triangles
    print(name, BUILD[arith], "depth", depth, "largest leaf", leaf, "nearest-first", near, "first-passing-child", first)
    assert leaf <= 31
    if name == "arms6":
        assert 40 <= depth <= 63 and first <= 64 and near >= 2 * first
    elif name == "bodyarms":
        assert near > 64 >= first
    else:
        assert depth == 64 and near > 64


@pytest.mark.parametrize("name", configs.DEEP)
def test_config_views_are_not_trivial(name):
    cfg = configs.CONFIGS[name]
    for rec in (load_golden(name)[1], load_ref_records(name)):
        assert len(rec["prim"]) == cfg["W"] * cfg["H"]
        dc.check_view(rec["prim"], rec["shadow"], cfg["mode"])
        assert np.isfinite(rec["rgb"]).all()


def _cap26_view(pkg, view, arith):
    """(cfg, fixture entry, basis12, sun) of a cap26 view in one build."""
    e = dc.load_cap26()["views"][view][BUILD[arith]]
    cfg = dc.cap26_cfg(view, None)
    return cfg, e, np.concatenate([dc.bits(e["eye"]), dc.bits(e["basis"])]).astype(np.float32), dc.bits(e["sun"])


@pytest.mark.parametrize("arith", ARITHS)
def test_cap26_host_builder_matches_the_reference(pkg, arith, cap26_obj):
    import oracle
    mesh, bvh = scene_of("cap26", arith, cap26_obj)
    want = dc.load_cap26()["scene_" + BUILD[arith]]
    assert (len(mesh), len(bvh.nodes)) == (want["n_tri"], want["n_nodes"])
    assert hashlib.sha256(mesh.tri.tobytes()).hexdigest() == want["tri48_sha256"]
    assert hashlib.sha256(mesh.norm.tobytes()).hexdigest() == want["norm36_sha256"]
    assert oracle.canonical_bvh_sha(bvh.nodes.reshape(-1), bvh.prim) == want["bvh_canonical_sha256"]


def check_cap26_frame(pkg, scene, view, arith, render=None):
    """A scene's frame of a cap26 view against the reference's: PPM sha256, rays, hits."""
    cfg, e, b12, sun = _cap26_view(pkg, view, arith)
    W, H = cfg["W"], cfg["H"]
    px, rgb, st = (render or scene.render)(b12, sun, W, H, mode=pkg.cfg_mode(cfg, arith))
    assert hashlib.sha256(pkg.ppm(W, H, rgb)).hexdigest() == e["ppm_sha256"], (view, BUILD[arith])
    assert (st["rays"], st["hits"]) == (e["rays"], e["hits"]), (view, BUILD[arith])
    assert np.isfinite(px).all()
    return px, rgb


def check_cap26_records(pkg, view, arith, prim, tuv, shadow):
    """Per-pixel records ([W*H] prim, [W*H, 3] t u v, [W*H] shadow: -1 miss, 0 lit, 1 occluded) against the stored sample."""
    r = _cap26_view(pkg, view, arith)[1]["records"]
    px = np.asarray(r["pixel"])
    want = np.asarray(r["prim"])
    assert np.array_equal(np.asarray(prim)[px], want)
    bits = np.asarray(r["tuv_bits"], np.uint32).reshape(-1, 3)
    assert np.array_equal(np.ascontiguousarray(tuv, np.float32).view(np.uint32).reshape(-1, 3)[px][want >= 0], bits[want >= 0])
    if shadow is not None:
        assert np.array_equal(np.asarray(shadow)[px], np.asarray(r["shadow"]))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("view", list(dc.CAP26_VIEWS))
def test_cap26_cpu_frames_and_records(pkg, view, arith, cap26_obj):
    mesh, bvh = scene_of("cap26", arith, cap26_obj)
    cfg, e, b12, sun = _cap26_view(pkg, view, arith)
    s = pkg.CpuScene(mesh, bvh)
    try:
        check_cap26_frame(pkg, s, view, arith)
        rays = pkg.camera_rays(b12, cfg["W"], cfg["H"], arith)
        qmode = pkg.cfg_mode(cfg, arith) & (pkg.MODE_FMA | pkg.MODE_ROBUST)
        _, _, hits, status, _ = s.shade(rays, sun, mode=qmode, pixels=True, hits=True, status=True)
    finally:
        s.close()
    shadow = status.astype(np.int32) - 1 if cfg["mode"] == "full" else None   # status: 0 miss, 1 lit, 2 shadowed
    dc.check_view(hits["prim"], shadow, cfg["mode"])
    check_cap26_records(pkg, view, arith, hits["prim"], np.stack([hits["t"], hits["u"], hits["v"]], 1), shadow)


@pytest.mark.parametrize("name", list(dc.MESHES) + ["arm1"])
def test_entry_cut(pkg, name, cap26_obj, tmp_path):
    """check_cut on every deep scene's table.  The cut splits its open node of largest area, so over six
    or 26 arms its 64 nodes spread: measured deepest LCA 11 (arms6), 7 (bodyarms), 8 (cap26) -- no
    deeper than the dragon's.  One arm alone (deep_common.arm1: 64 triangles, 63 inner nodes that the cut
    opens completely) is the chain that drives the table's 64-bit root paths (entry_cut.hpp) past bit
    30: there the deepest LCA must be at least 30 (measured: 35)."""
    if name == "arm1":
        p = tmp_path / "arm1.obj"
        p.write_bytes(dc.obj_text(dc.arm1()))
        mesh, bvh = _load(str(p), 1)
    else:
        mesh, bvh = scene_of(name, 1, cap26_obj)
    pairs, _, rlc = pkg.entry_relayout(mesh, bvh)
    cut = pkg.entry_cut(pairs, rlc, bvh.nodes[0, :6].copy().view(np.float32))
    assert not rlc and cut.n == min(64, len(pairs) + 1) and cut.entry_ok == 1
    E.check_cut(E.Tree(pairs, len(mesh)), cut)
    deepest = int(np.asarray(cut.depth)[:cut.n, :cut.n].max())
    print(name, "cut nodes", cut.n, "deepest LCA", deepest)
    assert deepest <= 63
    if name == "arm1":
        assert deepest >= 30


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def upkeep_view(pkg, name, arith):
    """(basis12, sun, W, H, mode) the upkeep tests render the moved mesh with: the 2^-20 zoom."""
    cfg = configs.CONFIGS["arms6_zoom20"] if name != "cap26" else dc.cap26_cfg("full", None)
    cam, sun = pkg.pose(cfg, arith=arith)
    return np.asarray(cam.basis(cfg["W"], cfg["H"]), np.float32), sun, cfg["W"], cfg["H"], pkg.cfg_mode(cfg, arith)


def cpu_answers(pkg, s, view):
    b12, sun, W, H, mode = view
    px, rgb, st = s.render(b12, sun, W, H, mode=mode)
    return dict(px=px, rgb=rgb, st={k: st[k] for k in ("rays", "hits", "node_pairs", "tri_tests")})


def assert_same(a, b):
    assert np.array_equal(_bits(a["px"]), _bits(b["px"])) and np.array_equal(a["rgb"], b["rgb"])
    assert a["st"] == b["st"]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(dc.MESHES))
def test_cpu_upkeep_equals_fresh_scenes(pkg, name, arith, cap26_obj):
    """Every arm scaled by its own power of two: refit, sah_cost, rebuild and update of a CpuScene against
    fresh scenes over the numpy-refitted and the rebuilt BVH."""
    mesh, bvh = scene_of(name, arith, cap26_obj)
    moved = dc.moved(pkg, mesh, name)
    view = upkeep_view(pkg, name, arith)
    refit_bvh = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim)
    rebuilt_bvh = pkg.build_bvh(moved, arith)
    assert dc.depth_and_leaf(rebuilt_bvh.nodes)[0] >= 40
    want = {}
    for k, b in (("refit", refit_bvh), ("rebuilt", rebuilt_bvh)):
        f = pkg.CpuScene(moved, b)
        try:
            want[k] = cpu_answers(pkg, f, view)
            qc.assert_cost(f.sah_cost(), b.nodes, k)
        finally:
            f.close()
    assert 10 * want["refit"]["st"]["hits"] >= view[2] * view[3], "the moved mesh left the view"
    assert want["refit"]["st"] != want["rebuilt"]["st"], "the rebuilt tree walks like the refitted one: nothing told apart"
    for how in ("refit", "rebuild", "update_keeps", "update_rebuilds"):
        s = pkg.CpuScene(mesh, bvh)
        try:
            if how == "refit":
                s.refit(moved)
            elif how == "rebuild":
                s.rebuild(moved, arith=arith)
            elif how == "update_keeps":
                assert s.update(moved, math.inf, arith=arith)["rebuilt"] == 0
            else:
                assert s.update(moved, 1e-9, arith=arith)["rebuilt"] == 1
            w = want["refit" if how in ("refit", "update_keeps") else "rebuilt"]
            assert_same(cpu_answers(pkg, s, view), w)
            qc.assert_cost(s.sah_cost(), (refit_bvh if w is want["refit"] else rebuilt_bvh).nodes, how)
        finally:
            s.close()
