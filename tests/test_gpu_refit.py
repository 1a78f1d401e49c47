"""Refit of a device scene (ceres_scene_refit / _device / _f64, scene_refit.hip): the scene after its
triangles moved -- leaf-ordered triangles regathered, every sibling-pair box, every shadow-BVH4 child box
and the root box recomputed, the quantised BVH4 copy dropped, topology kept.

Every comparison is against a FRESH scene that the existing constructors create from the moved triangles
and a BVH refitted in numpy (tests/refit_common.py), never against the refitted scene itself.  The fresh
scene's answers are computed once per scene and shared.  Each test creates its scenes and runs them once."""
import functools
import os
import subprocess

import numpy as np
import pytest

import refit_common as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def frame_answers(pkg, scene, basis, sun, W, H, mode):
    """render + records of a scene: the float framebuffer, RGB8, rays / hits and the per-pixel records."""
    px, rgb, st = scene.render(basis, sun, W, H, mode=mode)
    prim, tuv, sh, _ = scene.records(basis, sun, W, H, mode=mode)
    return dict(px=px, rgb=rgb, rays=st["rays"], hits=st["hits"], prim=prim, tuv=tuv, sh=sh)


def assert_frames_equal(a, b):
    for k in ("px", "rgb", "prim", "tuv", "sh"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert (a["rays"], a["hits"]) == (b["rays"], b["hits"])


@functools.lru_cache(maxsize=None)
def case(name, f64=False, W=None, H=None):
    """Inputs and the fresh scenes' answers of one config (exact arithmetic), shared by the tests."""
    from conftest import import_package
    pkg = import_package()
    mesh, bvh, moved, moved_bvh = rc.moved_scene_inputs(pkg, name, f64)
    basis, sun, W0, H0, mode = rc.pose_of(pkg, name, f64)
    if W:
        cam = (pkg.pose_f64 if f64 else pkg.pose)(pkg.configs.CONFIGS[name])[0]
        basis, W0, H0 = cam.basis(W, H), W, H
    c = dict(mesh=mesh, bvh=bvh, moved=moved, moved_bvh=moved_bvh, basis=basis, sun=sun, W=W0, H=H0, mode=mode)
    fresh = pkg.Scene(moved, moved_bvh)
    try:
        c["fresh"] = frame_answers(pkg, fresh, basis, sun, W0, H0, mode)
        c["fresh_boxes"] = fresh.read_boxes()
        rays = (pkg.camera_rays64 if f64 else pkg.camera_rays)(basis, W0, H0)
        c["rays"] = rays
        hits, occ, tst = fresh.trace(rays, closest=True, occluded=True)
        spx, srgb, shits, status, sst = fresh.shade(rays, sun, pixels=True, rgb8=True, hits=True, status=True)
        c["fresh_q"] = dict(hits=hits, occ=occ, spx=spx, srgb=srgb, shits=shits, status=status,
                            counts=(tst["rays"], tst["hits"], sst["rays"], sst["hits"]))
    finally:
        fresh.close()
    if not f64:
        st = pkg.Scene(moved, moved_bvh, stats=True)
        try:
            _, _, s = st.render(basis, sun, W0, H0, mode=mode | pkg.MODE_PRIMARY)
            c["fresh_primary_stats"] = (s["rays"], s["hits"], s["node_pairs"], s["tri_tests"])
        finally:
            st.close()
    return c


def queries(pkg, scene, c):
    hits, occ, tst = scene.trace(c["rays"], closest=True, occluded=True)
    spx, srgb, shits, status, sst = scene.shade(c["rays"], c["sun"], pixels=True, rgb8=True, hits=True, status=True)
    return dict(hits=hits, occ=occ, spx=spx, srgb=srgb, shits=shits, status=status,
                counts=(tst["rays"], tst["hits"], sst["rays"], sst["hits"]))


def assert_queries_equal(a, b):
    for k in ("hits", "occ", "spx", "srgb", "shits", "status"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["counts"] == b["counts"]


def device_scene(pkg, mesh, stats=False):
    """A Scene.from_device scene over a GPU-built BVH of `mesh` (tensors returned to keep them alive)."""
    import torch
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
    scene = pkg.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(),
                                  stats=stats, stream=stream)
    return scene, (d_tri, d_norm, d_nodes, d_prim)


def check_nodes4(nodes4, boxes, name):
    """Every non-empty BVH4 child box is one of the refitted BVH2 boxes; empty slots are inverted-infinite."""
    rows = nodes4.reshape(-1, 6, 4)                                    # record, {lo_x, hi_x, lo_y, hi_y, lo_z, hi_z}, child
    n_children = 0
    for rec in rows:
        for c in range(4):
            b = tuple(float(x) for x in rec[:, c])
            if b == (np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf):
                continue
            assert b in boxes, (name, b)
            n_children += 1
    assert n_children >= 2


def shared_box_records(nodes4):
    """Records with at least two non-empty children that all carry one box (piece nodes of an oversized leaf)."""
    out = []
    for k, rec in enumerate(nodes4.reshape(-1, 6, 4)):
        kids = [tuple(rec[:, c]) for c in range(4) if rec[0, c] != np.inf]
        if len(kids) >= 2 and len(set(kids)) == 1:
            out.append(k)
    return out


@pytest.mark.parametrize("first_order", [False, True])
@pytest.mark.parametrize("name", rc.SCENES)
def test_refit_host_scene(gpu, name, first_order):
    """Scene.refit on a host-created scene: frame, RGB8, rays / hits, records, trace and shade equal the
    fresh scene's; read_boxes: pair boxes equal the fresh host-created scene's elementwise (the host path
    numbers both alike), BVH4 child boxes are refitted BVH2 boxes, empty slots stay inverted-infinite and
    (dupleaf) the children of a piece record still share one box.  first_order: the scene's BVH4 children
    were permuted by order_shadow_bvh4 at creation (CERES_SCENE_FIRST_ORDER), and their box sources with them."""
    pkg = gpu
    c = case(name)
    s = pkg.Scene(c["mesh"], c["bvh"], first_order=first_order)
    try:
        pieces = shared_box_records(s.read_boxes()[1]) if name == "dupleaf" else []
        s.refit(c["moved"])
        got = frame_answers(pkg, s, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
        q = queries(pkg, s, c)
        pairs, nodes4 = s.read_boxes()
    finally:
        s.close()
    assert_frames_equal(got, c["fresh"])
    assert_queries_equal(q, c["fresh_q"])
    fp, _ = c["fresh_boxes"]
    assert pairs.shape == fp.shape and np.array_equal(pairs, fp)      # by value: a zero bound may carry either sign
    if name == "tri1":                                                 # the root is a leaf: no pair, no BVH4 record
        assert pairs.shape[0] == 0 and nodes4 is None
        return
    boxes = rc.box_set(c["moved_bvh"].nodes)
    check_nodes4(nodes4, boxes, name)
    if name == "dupleaf":
        assert pieces and set(pieces) <= set(shared_box_records(nodes4))
        for k in pieces:
            assert tuple(float(x) for x in nodes4[k].reshape(6, 4)[:, 0]) in boxes


@pytest.mark.parametrize("name", rc.SCENES)
def test_refit_device_scene(gpu, name):
    """Scene.refit_device on a Scene.from_device scene built through build_bvh_device (records numbered
    by the device relayout): the same frame, records and queries; its BVH4 child boxes are refitted
    BVH2 boxes too."""
    import torch
    pkg = gpu
    c = case(name)
    s, keep = device_scene(pkg, c["mesh"])
    try:
        d_tri = torch.from_numpy(c["moved"].tri.reshape(-1).copy()).to("cuda:0")
        d_norm = torch.from_numpy(c["moved"].norm.reshape(-1).copy()).to("cuda:0")
        s.refit_device(d_tri.data_ptr(), d_norm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        got = frame_answers(pkg, s, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
        q = queries(pkg, s, c)
        pairs, nodes4 = s.read_boxes()
    finally:
        s.close()
    del keep
    assert_frames_equal(got, c["fresh"])
    assert_queries_equal(q, c["fresh_q"])
    if name != "tri1":
        boxes = rc.box_set(c["moved_bvh"].nodes)
        check_nodes4(nodes4, boxes, name)
        assert {tuple(float(x) for x in r[:6]) for r in pairs} | {tuple(float(x) for x in r[6:]) for r in pairs} <= boxes


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name", rc.SCENES)
def test_refit_pins_the_traversal_counters(gpu, name, kind):
    """stats=True scenes in primary-only mode: node_pairs and tri_tests equal the fresh scene's -- the
    pair boxes are pinned, not just the picture."""
    import torch
    pkg = gpu
    c = case(name)
    keep = None
    if kind == "host":
        s = pkg.Scene(c["mesh"], c["bvh"], stats=True)
    else:
        s, keep = device_scene(pkg, c["mesh"], stats=True)
    try:
        if kind == "host":
            s.refit(c["moved"])
        else:
            d_tri = torch.from_numpy(c["moved"].tri.reshape(-1).copy()).to("cuda:0")
            s.refit_device(d_tri.data_ptr(), 0)
        _, _, st = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"] | pkg.MODE_PRIMARY)
    finally:
        s.close()
    del keep
    assert (st["rays"], st["hits"], st["node_pairs"], st["tri_tests"]) == c["fresh_primary_stats"]


def test_batch_render_after_refit_with_the_cull(gpu):
    """render_batch_device, 4 frames of the bunny's orbit at 160x120 (the background cull active), after a
    refit that moves part of the body outside the OLD root box: each frame equals the fresh scene's -- a
    stale root box or cull rectangle would cut the body off."""
    import torch
    pkg = gpu
    name = "bunny_orbit7_160x120"
    c = case(name)
    cfg = pkg.configs.CONFIGS[name]
    old_root = rc.node_fields(c["bvh"].nodes)[0][0]
    new_root = rc.node_fields(c["moved_bvh"].nodes)[0][0]
    assert np.any(new_root[0::2] < old_root[0::2]) or np.any(new_root[1::2] > old_root[1::2])
    cam, sun = pkg.pose(cfg)
    W, H, F = c["W"], c["H"], 4
    b12, s3 = pkg.orbit_cameras(cam, sun, W, H, F, axis=cfg["orbit"][0], step_deg=cfg["orbit"][1], rotate_first=False)

    def batch(scene):
        px = torch.empty(F * 3 * W * H, dtype=torch.float32, device="cuda")
        rgb = torch.empty(F * 3 * W * H, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        scene.render_batch_device(b12, s3, W, H, mode=c["mode"], d_pixels=px.data_ptr(), d_rgb8=rgb.data_ptr(),
                                  d_counters=cnt.data_ptr())
        torch.cuda.synchronize()
        return px.cpu().numpy().reshape(F, -1), rgb.cpu().numpy().reshape(F, -1), cnt.cpu().numpy()[:2]

    s = pkg.Scene(c["mesh"], c["bvh"])
    fresh = pkg.Scene(c["moved"], c["moved_bvh"])
    try:
        batch(s)                                                      # the cull rectangle of the old box has been in use
        s.refit(c["moved"])
        a = batch(s)
        b = batch(fresh)
        single = [fresh.render(b12[f], s3[f], W, H, mode=c["mode"]) for f in range(F)]
    finally:
        s.close()
        fresh.close()
    for f in range(F):
        assert np.array_equal(a[0][f].view(np.uint32), b[0][f].view(np.uint32)), f
        assert np.array_equal(a[1][f], b[1][f]), f
        assert np.array_equal(a[0][f].view(np.uint32), single[f][0].view(np.uint32)), f
        assert np.count_nonzero(a[1][f]) > 0
    assert tuple(a[2]) == tuple(b[2])


def test_qbvh4_is_requantised_after_a_refit(gpu):
    """CERES_MODE_QBVH4 rendered before and after a refit: the frame after equals the fresh scene's
    CERES_MODE_QBVH4 frame (a stale quantised copy would keep the old boxes)."""
    pkg = gpu
    c = case("bunny_orbit7_160x120")
    mode = c["mode"] | pkg.MODE_QBVH4
    s = pkg.Scene(c["mesh"], c["bvh"])
    fresh = pkg.Scene(c["moved"], c["moved_bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
        s.refit(c["moved"])
        a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
        b = fresh.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
    finally:
        s.close()
        fresh.close()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert (a[2]["rays"], a[2]["hits"]) == (b[2]["rays"], b[2]["hits"])
    assert not np.array_equal(before[1], a[1])


@pytest.mark.parametrize("name,W,H", [("bunny_orbit7_160x120", 97, 61), ("tri1", None, None)])
def test_refit_double_scene(gpu, name, W, H):
    """Double scenes (pairs and leaf-ordered triangles only): refit, then render / records / trace / shade
    equal the fresh double scene's; the pair boxes equal the fresh scene's."""
    pkg = gpu
    c = case(name, True, W, H)
    s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        s.refit(c["moved"])
        got = frame_answers(pkg, s, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
        q = queries(pkg, s, c)
        pairs, nodes4 = s.read_boxes()
    finally:
        s.close()
    assert_frames_equal(got, c["fresh"])
    assert_queries_equal(q, c["fresh_q"])
    assert nodes4 is None and pairs.dtype == np.float64 and np.array_equal(pairs, c["fresh_boxes"][0])
    assert np.count_nonzero(got["prim"] >= 0) * 10 >= got["prim"].size


def test_refit_double_scene_from_device_arrays(gpu):
    """ceres_scene_refit_f64_device: the moved double triangles and normals taken from device memory."""
    import torch
    pkg = gpu
    c = case("bunny_orbit7_160x120", True, 97, 61)
    s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        d_tri = torch.from_numpy(c["moved"].tri.reshape(-1).copy()).to("cuda:0")
        d_norm = torch.from_numpy(c["moved"].norm.reshape(-1).copy()).to("cuda:0")
        s.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
        got = frame_answers(pkg, s, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
    finally:
        s.close()
    assert_frames_equal(got, c["fresh"])


@pytest.mark.parametrize("kind", ["host", "device"])
def test_two_refits_equal_one(gpu, kind):
    """Deformed, then deformed again with other constants: the frames are those of one refit to the last
    mesh (level lists, staging and root-box state of the first refit are reused, not stale)."""
    import torch
    pkg = gpu
    name = "bunny_orbit7_160x120"
    c = case(name)
    last = rc.deform(c["mesh"], **rc.OTHER)
    last_bvh = pkg.Bvh(rc.refit_nodes(c["bvh"].nodes, c["bvh"].prim, last.tri), c["bvh"].prim)
    keep = None
    if kind == "host":
        s = pkg.Scene(c["mesh"], c["bvh"])
    else:
        s, keep = device_scene(pkg, c["mesh"])
    fresh = pkg.Scene(last, last_bvh)
    try:
        for m in (c["moved"], last):
            if kind == "host":
                s.refit(m)
            else:
                d_tri = torch.from_numpy(m.tri.reshape(-1).copy()).to("cuda:0")
                d_norm = torch.from_numpy(m.norm.reshape(-1).copy()).to("cuda:0")
                s.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
        got = frame_answers(pkg, s, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
        want = frame_answers(pkg, fresh, c["basis"], c["sun"], c["W"], c["H"], c["mode"])
    finally:
        s.close()
        fresh.close()
    del keep
    assert_frames_equal(got, want)
    assert not np.array_equal(got["rgb"], c["fresh"]["rgb"])


def test_refit_errors_leave_the_scene_untouched(gpu):
    """A wrong n_tri, a float / double mismatch, a null or misaligned triangle pointer: CERES_EINVAL, and the
    scene renders its old frame."""
    import ctypes
    import torch
    pkg = gpu
    c = case("quad")
    d = case("tri1", True)
    L = pkg.lib()
    s = pkg.Scene(c["mesh"], c["bvh"])
    s64 = pkg.Scene(d["mesh"], d["bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        m = c["moved"]
        with pytest.raises(pkg.CeresError):
            s.refit(pkg.Mesh(m.tri[:-1], m.norm[:-1]))
        with pytest.raises(pkg.CeresError):
            s.refit(d["moved"])
        assert L.ceres_scene_refit_f64(s._h, pkg._p(d["moved"].tri, ctypes.c_double), len(m), None) == -1
        assert L.ceres_scene_refit(s64._h, pkg._p(m.tri, ctypes.c_float), len(d["moved"]), None) == -1
        assert L.ceres_scene_refit(s._h, None, len(m), None) == -1
        d_tri = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), m.tri.reshape(-1)])).to("cuda:0")
        with pytest.raises(pkg.CeresError):
            s.refit_device(d_tri.data_ptr() + 4)
        with pytest.raises(pkg.CeresError):
            s.refit_device(d_tri.data_ptr(), n_tri=len(m) + 1)
        after = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
        s64.close()
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("double", [False, True])
def test_cli_refit_on_the_gpu(gpu, tmp_path, double):
    """./render A.obj --refit B.obj [--double] on the GPU writes the PPM of a fresh scene of B over A's
    refitted BVH (B written by the test's OBJ writer, read back by the library's loader)."""
    pkg = gpu
    name = "dupleaf"
    cfg = pkg.configs.CONFIGS[name]
    arith = pkg.ARITH_FMA                                                  # the CLI's default arithmetic
    mesh, bvh, _ = pkg.prepare(cfg, f64=double, arith=arith)
    b_obj = str(tmp_path / "b.obj")
    rc.write_obj(b_obj, rc.deform(pkg.prepare(cfg, arith=arith)[0]))
    moved = (pkg.load_obj_f64 if double else pkg.load_obj)(b_obj, arith)
    basis, sun, W, H, mode = rc.pose_of(pkg, name, double, arith)
    fresh = pkg.Scene(moved, pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim))
    try:
        _, rgb, st = fresh.render(basis, sun, W, H, mode=mode)
    finally:
        fresh.close()
    out = str(tmp_path / "out.ppm")
    r = subprocess.run([pkg.CLI_PATH] + pkg.configs.cli_args(cfg) + ["--refit", b_obj, "-o", out] + (["--double"] if double else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == pkg.ppm(W, H, rgb)
    assert "Rays: %d\tHits: %d" % (st["rays"], st["hits"]) in r.stdout
    r = subprocess.run([pkg.CLI_PATH, pkg.configs.obj_path(cfg), "--refit", os.path.join(os.path.dirname(__file__), "golden", "quad.obj"),
                        "--size", "8", "8", "-o", str(tmp_path / "x.ppm")] + (["--double"] if double else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "face count" in r.stderr
