"""Upkeep of a device scene (scene_quality.hip): ceres_scene_sah_cost, the in-place rebuild
(ceres_scene_rebuild / _device) and the refit-or-rebuild call (ceres_scene_update / _device).

Costs are compared with the numpy model of tests/quality_common.py on reference-layout nodes, within the
bound derived there.  A rebuilt scene is compared with a FRESH Scene.from_device scene over a GPU-built BVH
of the moved mesh -- bit for bit: frames, records, queries, ceres_scene_info, the shadow stacks, the box
readback and the cost.  The fresh scenes' answers are computed once per scene and shared; each test creates
its scenes and runs them once."""
import ctypes
import functools
import math

import numpy as np
import pytest

import quality_common as qc
import refit_common as rc

pytestmark = pytest.mark.gpu

BUNNY = "bunny_orbit7_160x120"
EUNSUPPORTED, EINVAL = -6, -1


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def frame_answers(scene, c, mode=None):
    mode = c["mode"] if mode is None else mode
    px, rgb, st = scene.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
    prim, tuv, sh, _ = scene.records(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
    return dict(px=px, rgb=rgb, rays=st["rays"], hits=st["hits"], prim=prim, tuv=tuv, sh=sh)


def assert_frames_equal(a, b):
    for k in ("px", "rgb", "prim", "tuv", "sh"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert (a["rays"], a["hits"]) == (b["rays"], b["hits"])


def queries(pkg, scene, c):
    rays = pkg.camera_rays(c["basis"], c["W"], c["H"])
    hits, occ, tst = scene.trace(rays, closest=True, occluded=True)
    spx, srgb, shits, status, sst = scene.shade(rays, c["sun"], pixels=True, rgb8=True, hits=True, status=True)
    return dict(hits=hits, occ=occ, spx=spx, srgb=srgb, shits=shits, status=status,
                counts=(tst["rays"], tst["hits"], sst["rays"], sst["hits"]))


def assert_queries_equal(a, b):
    for k in ("hits", "occ", "spx", "srgb", "shits", "status"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["counts"] == b["counts"]


def everything(pkg, scene, c):
    """All a rebuilt scene must share with the fresh one."""
    pairs, nodes4 = scene.read_boxes()
    return dict(frame=frame_answers(scene, c), q=queries(pkg, scene, c), info=scene.info(), pairs=pairs, nodes4=nodes4,
                cost=scene.sah_cost())


def assert_everything_equal(a, b):
    assert_frames_equal(a["frame"], b["frame"])
    assert_queries_equal(a["q"], b["q"])
    assert a["info"] == b["info"]
    assert a["pairs"].shape == b["pairs"].shape and np.array_equal(bits(a["pairs"]), bits(b["pairs"]))
    assert (a["nodes4"] is None) == (b["nodes4"] is None)
    if a["nodes4"] is not None:
        assert a["nodes4"].shape == b["nodes4"].shape and np.array_equal(bits(a["nodes4"]), bits(b["nodes4"]))
    assert qc.dbits(a["cost"]) == qc.dbits(b["cost"])


def to_device(mesh):
    import torch
    return (torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0"), torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0"))


def device_scene(pkg, mesh, stats=False, first_order=False):
    """A ceres_scene_create_device scene over a GPU-built BVH of `mesh` (tensors returned to keep them alive)."""
    import torch
    n = len(mesh)
    d_tri, d_norm = to_device(mesh)
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
    flags = (pkg.SCENE_STATS if stats else 0) | (pkg.SCENE_FIRST_ORDER if first_order else 0)
    h = pkg.lib().ceres_scene_create_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), 0,
                                            flags, stream or None)
    assert h, pkg.lib().ceres_last_error()
    return pkg.Scene(None, None, _handle=(h, 0, n)), (d_tri, d_norm, d_nodes, d_prim)


@functools.lru_cache(maxsize=None)
def fresh_device(name):
    """Everything of the fresh device scene of the MOVE mesh, computed once."""
    from conftest import import_package
    pkg = import_package()
    c = qc.inputs(name)
    s, keep = device_scene(pkg, c["moved"])
    try:
        return everything(pkg, s, c)
    finally:
        s.close()
        del keep


@functools.lru_cache(maxsize=None)
def fresh_refit(name):
    """Frame and queries of the fresh host scene of the MOVE mesh over the numpy-refitted BVH."""
    from conftest import import_package
    pkg = import_package()
    c = qc.inputs(name)
    s = pkg.Scene(c["moved"], c["moved_bvh"])
    try:
        return dict(frame=frame_answers(s, c), q=queries(pkg, s, c))
    finally:
        s.close()


def small_frame(pkg, c, name, f64):
    """A double scene's case at 97 x 61 (the double kernels are the slow ones)."""
    if not f64:
        return c
    cam = pkg.pose_f64(pkg.configs.CONFIGS[name])[0]
    return dict(c, basis=cam.basis(97, 61), W=97, H=61)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", rc.SCENES)
def test_cost_of_host_created_scenes(gpu, name, f64):
    """Float and double host-created scenes: the cost matches the model as built and after a refit, two
    calls return equal bits, and a render after the query equals the render before."""
    pkg = gpu
    c = small_frame(pkg, qc.inputs(name, f64), name, f64)
    s = pkg.Scene(c["mesh"], c["bvh"])
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
    assert (before[2]["rays"], before[2]["hits"]) == (after[2]["rays"], after[2]["hits"])
    if name == "tri1":
        assert built == 1.0 and refitted == 1.0


@pytest.mark.parametrize("name", rc.SCENES)
def test_cost_of_device_created_scenes(gpu, name):
    """Scene.from_device scenes (records numbered by the device relayout): the same model values -- the
    GPU builder makes the host builder's topology and boxes."""
    import torch
    pkg = gpu
    c = qc.inputs(name)
    s, keep = device_scene(pkg, c["mesh"])
    try:
        built, again = s.sah_cost(), s.sah_cost(stream=torch.cuda.current_stream().cuda_stream)
        d_tri, d_norm = to_device(c["moved"])
        s.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
        refitted = s.sah_cost()
    finally:
        s.close()
    del keep
    qc.assert_cost(built, c["bvh"].nodes, "as built")
    qc.assert_cost(refitted, c["moved_bvh"].nodes, "after the refit")
    assert qc.dbits(built) == qc.dbits(again)


@pytest.mark.parametrize("first_order", [False, True])
@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("name", rc.SCENES)
def test_rebuild_device_equals_a_fresh_device_scene(gpu, name, kind, first_order):
    """rebuild_device on a device-created and on a host-created scene, with and without
    CERES_SCENE_FIRST_ORDER: framebuffer, RGB8, rays / hits, records, trace, shade, info(), the shadow
    stacks, the box readback and the cost are the fresh Scene.from_device scene's, bit for bit; the cost
    matches the model on the host builder's BVH of the moved mesh."""
    import torch
    pkg = gpu
    c = qc.inputs(name)
    keep = None
    if kind == "device":
        s, keep = device_scene(pkg, c["mesh"], first_order=first_order)
    else:
        s = pkg.Scene(c["mesh"], c["bvh"], first_order=first_order)
    try:
        d_tri, d_norm = to_device(c["moved"])
        s.rebuild_device(d_tri.data_ptr(), d_norm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        got = everything(pkg, s, c)
    finally:
        s.close()
    del keep
    assert_everything_equal(got, fresh_device(name))
    qc.assert_cost(got["cost"], c["rebuilt_bvh"].nodes, "rebuilt")


@pytest.mark.parametrize("name", rc.SCENES)
def test_rebuild_from_host_arrays(gpu, name):
    """Scene.rebuild(mesh): the same scene from host arrays."""
    pkg = gpu
    c = qc.inputs(name)
    s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        s.rebuild(c["moved"])
        got = everything(pkg, s, c)
    finally:
        s.close()
    assert_everything_equal(got, fresh_device(name))


def test_rebuild_keeps_normals_when_none_are_given(gpu):
    """d_norm = 0 keeps the scene's normals: the frame is the fresh device scene's of the moved triangles
    with the OLD normals."""
    pkg = gpu
    c = qc.inputs("dupleaf")
    s, keep = device_scene(pkg, c["mesh"])
    old, keep2 = device_scene(pkg, pkg.Mesh(c["moved"].tri, c["mesh"].norm))
    try:
        d_tri, _ = to_device(c["moved"])
        s.rebuild_device(d_tri.data_ptr())
        a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        b = old.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
    finally:
        s.close()
        old.close()
    del keep, keep2
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert not np.array_equal(bits(a[0]), bits(fresh_device("dupleaf")["frame"]["px"]))


def test_refits_around_a_rebuild(gpu):
    """A refit BEFORE the rebuild (its level list is of the old topology) and one AFTER it, back to the
    original mesh: the scene equals a fresh Scene(mesh, refit_nodes(nb)) with nb = build_bvh(moved)."""
    pkg = gpu
    c = qc.inputs(BUNNY)
    nb = c["rebuilt_bvh"]
    back = pkg.Bvh(rc.refit_nodes(nb.nodes, nb.prim, c["mesh"].tri), nb.prim)
    s = pkg.Scene(c["mesh"], c["bvh"])
    fresh = pkg.Scene(c["mesh"], back)
    try:
        s.refit(c["other"])
        s.rebuild(c["moved"])
        s.refit(c["mesh"])
        got = dict(frame=frame_answers(s, c), q=queries(pkg, s, c), cost=s.sah_cost())
        want = dict(frame=frame_answers(fresh, c), q=queries(pkg, fresh, c))
    finally:
        s.close()
        fresh.close()
    assert_frames_equal(got["frame"], want["frame"])
    assert_queries_equal(got["q"], want["q"])
    qc.assert_cost(got["cost"], back.nodes, "refitted back")


def test_qbvh4_is_requantised_after_a_rebuild(gpu):
    """CERES_MODE_QBVH4 rendered before and after a rebuild: the frame after is the fresh scene's
    CERES_MODE_QBVH4 frame (a stale quantised copy would keep the old records)."""
    pkg = gpu
    c = qc.inputs(BUNNY)
    mode = c["mode"] | pkg.MODE_QBVH4
    s = pkg.Scene(c["mesh"], c["bvh"])
    fresh, keep = device_scene(pkg, c["moved"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
        s.rebuild(c["moved"])
        a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
        b = fresh.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
    finally:
        s.close()
        fresh.close()
    del keep
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert (a[2]["rays"], a[2]["hits"]) == (b[2]["rays"], b[2]["hits"])
    assert not np.array_equal(before[1], a[1])


def test_batch_render_around_a_rebuild(gpu):
    """A 2-frame render_batch_device at one shape before and after a rebuild: the frames after are the
    fresh scene's -- the cached tile order is reused and the compacting launch culls with the NEW root box."""
    import torch
    pkg = gpu
    c = qc.inputs(BUNNY)
    cfg = pkg.configs.CONFIGS[BUNNY]
    cam, sun = pkg.pose(cfg)
    W, H, F = c["W"], c["H"], 2
    b12, s3 = pkg.orbit_cameras(cam, sun, W, H, F, axis=cfg["orbit"][0], step_deg=cfg["orbit"][1], rotate_first=False)

    def batch(scene):
        px = torch.empty(F * 3 * W * H, dtype=torch.float32, device="cuda")
        rgb = torch.empty(F * 3 * W * H, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        scene.render_batch_device(b12, s3, W, H, mode=c["mode"], d_pixels=px.data_ptr(), d_rgb8=rgb.data_ptr(),
                                  d_counters=cnt.data_ptr())
        torch.cuda.synchronize()
        return px.cpu().numpy().reshape(F, -1), rgb.cpu().numpy().reshape(F, -1), cnt.cpu().numpy()

    s = pkg.Scene(c["mesh"], c["bvh"])
    fresh, keep = device_scene(pkg, c["moved"])
    try:
        batch(s)
        s.rebuild(c["moved"])
        a = batch(s)
        b = batch(fresh)
    finally:
        s.close()
        fresh.close()
    del keep
    for f in range(F):
        assert np.array_equal(bits(a[0][f]), bits(b[0][f])), f
        assert np.array_equal(a[1][f], b[1][f]), f
        assert np.count_nonzero(a[1][f]) > 0
    assert tuple(a[2][:2]) == tuple(b[2][:2]) and a[2][6] == 0


def test_rebuild_pins_the_traversal_counters(gpu):
    """stats=True scenes in primary-only mode: node_pairs and tri_tests after a rebuild equal the fresh
    stats scene's -- the records are pinned, not just the picture."""
    pkg = gpu
    c = qc.inputs(BUNNY)
    mode = c["mode"] | pkg.MODE_PRIMARY
    s = pkg.Scene(c["mesh"], c["bvh"], stats=True)
    fresh, keep = device_scene(pkg, c["moved"], stats=True)
    try:
        s.rebuild(c["moved"])
        _, _, a = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
        _, _, b = fresh.render(c["basis"], c["sun"], c["W"], c["H"], mode=mode)
    finally:
        s.close()
        fresh.close()
    del keep
    keys = ("rays", "hits", "node_pairs", "tri_tests")
    assert [a[k] for k in keys] == [b[k] for k in keys] and a["node_pairs"] > 0


def close(got, nodes):
    want = qc.model_cost(nodes)
    return abs(got - want) <= qc.tolerance(nodes) * want


@pytest.mark.parametrize("name", rc.SCENES)
def test_update_never_rebuilds_at_infinity(gpu, name):
    """Scene.update with max_ratio = +inf: rebuilt == 0, the answers are the fresh scene's over the
    refitted BVH, the info fields match the model."""
    pkg = gpu
    c = qc.inputs(name)
    s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        u = s.update(c["moved"], math.inf)
        got = dict(frame=frame_answers(s, c), q=queries(pkg, s, c))
    finally:
        s.close()
    print(u)
    assert u["rebuilt"] == 0 and close(u["built_cost"], c["bvh"].nodes) and close(u["cost"], c["moved_bvh"].nodes)
    assert qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
    assert_frames_equal(got["frame"], fresh_refit(name)["frame"])
    assert_queries_equal(got["q"], fresh_refit(name)["q"])


@pytest.mark.parametrize("kind", ["device", "host"])
@pytest.mark.parametrize("name", rc.SCENES)
def test_update_rebuilds_below_the_ratio(gpu, name, kind):
    """max_ratio = 0.9 r: rebuilt == 1 and the scene is the fresh device scene of the moved mesh
    (update_device on a device-created scene, update on a host-created one); a second update with OTHER
    reports the rebuilt tree's cost as its baseline."""
    import torch
    pkg = gpu
    c = qc.inputs(name)
    keep = None
    if kind == "device":
        s, keep = device_scene(pkg, c["mesh"])
    else:
        s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        if kind == "device":
            d_tri, d_norm = to_device(c["moved"])
            u = s.update_device(d_tri.data_ptr(), 0.9 * c["r"], d_norm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        else:
            u = s.update(c["moved"], 0.9 * c["r"])
        got = everything(pkg, s, c)
        v = s.update(c["other"], math.inf)
    finally:
        s.close()
    del keep
    print(u, v)
    assert u["rebuilt"] == 1 and close(u["built_cost"], c["bvh"].nodes) and close(u["cost"], c["moved_bvh"].nodes)
    assert close(u["new_cost"], c["rebuilt_bvh"].nodes) and qc.dbits(u["new_cost"]) == qc.dbits(got["cost"])
    assert_everything_equal(got, fresh_device(name))
    assert v["rebuilt"] == 0 and qc.dbits(v["built_cost"]) == qc.dbits(u["new_cost"]) and close(v["cost"], c["other_bvh"].nodes)


@pytest.mark.parametrize("name", rc.SCENES)
def test_update_keeps_the_tree_above_the_ratio(gpu, name):
    """update_device with max_ratio = 1.1 r on a host-created scene keeps the tree: rebuilt == 0, the frame
    is the refitted scene's and the record count is still the host layout's."""
    pkg = gpu
    c = qc.inputs(name)
    s = pkg.Scene(c["mesh"], c["bvh"])
    try:
        n_pairs = s.info()["n_pairs"]
        d_tri, d_norm = to_device(c["moved"])
        u = s.update_device(d_tri.data_ptr(), 1.1 * c["r"], d_norm.data_ptr())
        got = frame_answers(s, c)
        info = s.info()
    finally:
        s.close()
    assert u["rebuilt"] == 0 and close(u["cost"], c["moved_bvh"].nodes) and qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
    assert close(u["built_cost"], c["bvh"].nodes) and info["n_pairs"] == n_pairs
    assert_frames_equal(got, fresh_refit(name)["frame"])


def test_refusals_leave_the_scene_untouched(gpu):
    """A double GPU scene: CERES_EUNSUPPORTED from rebuild and update (host and device calls); a device
    triangle pointer off 16-byte alignment, a wrong count, a bad arith or max_ratio, null pointers:
    CERES_EINVAL.  Both scenes render their old frames afterwards."""
    import torch
    pkg = gpu
    c = qc.inputs("quad")
    d = small_frame(pkg, qc.inputs("tri1", True), "tri1", True)
    L = pkg.lib()
    s = pkg.Scene(c["mesh"], c["bvh"])
    s64 = pkg.Scene(d["mesh"], d["bvh"])
    try:
        before = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        before64 = s64.render(d["basis"], d["sun"], d["W"], d["H"], mode=d["mode"])
        m, m64 = c["moved"], d["moved"]
        n = len(m)
        d_tri = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), m.tri.reshape(-1)])).to("cuda:0")
        d64 = torch.from_numpy(m64.tri.reshape(-1).copy()).to("cuda:0")
        tri = pkg._p(m.tri, ctypes.c_float)
        tri64 = ctypes.cast(pkg._p(m64.tri, ctypes.c_double), ctypes.POINTER(ctypes.c_float))
        info = pkg._UpdateInfo()
        unsupported = [
            L.ceres_scene_rebuild(s64._h, tri64, len(m64), None, 0),
            L.ceres_scene_update(s64._h, tri64, len(m64), None, 0, 2.0, ctypes.byref(info)),
            L.ceres_scene_rebuild_device(s64._h, d64.data_ptr(), len(m64), None, 0, None),
            L.ceres_scene_update_device(s64._h, d64.data_ptr(), len(m64), None, 0, math.inf, None, None),
        ]
        invalid = [
            L.ceres_scene_rebuild_device(s._h, d_tri.data_ptr() + 4, n, None, 0, None),
            L.ceres_scene_update_device(s._h, d_tri.data_ptr() + 4, n, None, 0, 2.0, None, None),
            L.ceres_scene_rebuild(s._h, tri, n + 1, None, 0), L.ceres_scene_update(s._h, tri, n - 1, None, 0, 2.0, None),
            L.ceres_scene_rebuild(s._h, None, n, None, 0), L.ceres_scene_update(None, tri, n, None, 0, 2.0, None),
            L.ceres_scene_rebuild(s._h, tri, n, None, 5), L.ceres_scene_update(s._h, tri, n, None, 5, 2.0, None),
            L.ceres_scene_update(s._h, tri, n, None, 0, math.nan, None), L.ceres_scene_update(s._h, tri, n, None, 0, 0.0, None),
            L.ceres_scene_update(s._h, tri, n, None, 0, -2.0, None),
            L.ceres_scene_sah_cost(None, ctypes.byref(ctypes.c_double()), None), L.ceres_scene_sah_cost(s._h, None, None),
        ]
        with pytest.raises(pkg.CeresError):
            s64.rebuild(m64)
        with pytest.raises(pkg.CeresError):
            s64.update(m64, 2.0)
        after = s.render(c["basis"], c["sun"], c["W"], c["H"], mode=c["mode"])
        after64 = s64.render(d["basis"], d["sun"], d["W"], d["H"], mode=d["mode"])
    finally:
        s.close()
        s64.close()
    assert unsupported == [EUNSUPPORTED] * 4, unsupported
    assert invalid == [EINVAL] * len(invalid), invalid
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert np.array_equal(bits(before64[0]), bits(after64[0])) and np.array_equal(before64[1], after64[1])


def test_cli_rebuild_above_on_the_gpu(gpu, tmp_path):
    """./render A.obj --refit B.obj --rebuild-above 1e-9 on the GPU writes the PPM of ./render B.obj --gpu-bvh
    and says `rebuilt` -- with --gpus 2 once per rank, the same PPM; with --double the library refuses
    (status 1, its message)."""
    import subprocess
    pkg = gpu
    cfg = pkg.configs.CONFIGS["dupleaf"]
    a_args = pkg.configs.cli_args(cfg)
    b_obj = str(tmp_path / "b.obj")
    rc.write_obj(b_obj, rc.deform(pkg.prepare(cfg, arith=pkg.ARITH_FMA)[0]))
    b_args = [b_obj if x == pkg.configs.obj_path(cfg) else x for x in a_args]

    def cli(args):
        return subprocess.run([pkg.CLI_PATH] + args, capture_output=True, text=True, timeout=120)

    rb = cli(b_args + ["--gpu-bvh", "-o", str(tmp_path / "b.ppm")])
    ra = cli(a_args + ["--refit", b_obj, "--rebuild-above", "1e-9", "-o", str(tmp_path / "a.ppm")])
    assert rb.returncode == 0 and ra.returncode == 0, (rb.stderr, ra.stderr)
    assert open(str(tmp_path / "a.ppm"), "rb").read() == open(str(tmp_path / "b.ppm"), "rb").read()
    lines = [ln for ln in ra.stdout.splitlines() if ln.startswith("SAH cost")]
    assert len(lines) == 1 and lines[0].endswith("rebuilt")
    r2 = cli(a_args + ["--gpus", "2", "--refit", b_obj, "--rebuild-above", "1e-9", "-o", str(tmp_path / "a2.ppm")])
    assert r2.returncode == 0, r2.stderr
    assert open(str(tmp_path / "a2.ppm"), "rb").read() == open(str(tmp_path / "b.ppm"), "rb").read()
    lines = [ln for ln in r2.stdout.splitlines() if ln.startswith("SAH cost")]
    assert len(lines) == 2 and all(ln.endswith("rebuilt") for ln in lines)          # every rank's scene copy
    r = cli(a_args + ["--double", "--refit", b_obj, "--rebuild-above", "2", "-o", str(tmp_path / "d.ppm")])
    assert r.returncode == 1 and "double" in r.stderr
