"""Retired tiles on the device: in a batch launch with entry nodes, a tile that is root-culled or
that no cut rectangle reaches is written by the fill workgroups, and a wavefront group of such
tiles leaves at once (render_hip.hip: live_mask_row, fill_retired_runs, ceres_order_compact's flag
bytes, the tile path of ceres_fused).

Image parity by the method of test_gpu_tile_compact.py: every byte of the float framebuffer and of
the RGB8 body (pre-filled with 0xA5, 64 guard bytes behind them) and the ray / hit / primary /
shadow counts of the production batch equal the same frames one per launch on a CERES_SCENE_STATS
scene, which never culls, compacts or retires; the error word is 0.  The read-back live mask and
group flags (ceres_debug_retire) equal tests/retire_model.py's, computed from the scene's own cut
table as the device holds it."""
import numpy as np
import pytest

import configs
import cull_fill_model as M
import retire_model as R
import tile_compact_model as C


class _Env:
    pass


def _scene_env(pkg, mesh, bvh):
    s = _Env()
    s.mesh, s.bvh = mesh, bvh
    s.prod, s.ref = pkg.Scene(mesh, bvh), pkg.Scene(mesh, bvh, stats=True)
    s.root = M.root_box(mesh.tri)
    s.refs = {}
    return s


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    e = _Env()
    e.pkg = pkg
    cfg = configs.CONFIGS["bunny_1080"]
    mesh, bvh, _ = pkg.prepare(cfg, arith=pkg.ARITH_FMA)
    e.sun = np.asarray(cfg["sun"], np.float32)
    e.full = pkg.MODE_FULL | pkg.MODE_FMA
    e.scenes = {"bunny": _scene_env(pkg, mesh, bvh), "two": _scene_env(pkg, *R.two_patches(pkg))}
    yield e
    for s in e.scenes.values():
        s.prod.close()
        s.ref.close()


def _views(e, s, name, W, H):
    """The frames of a batch: named views of tile_compact_model (bunny), looks at the two patches."""
    if name == "bunny":
        cams = C.cameras(e.pkg, s.root, W, H)
        names = ("odd", "gone", "centre") if W == 136 else ("odd", "gone") if W == 1024 else ("inside", "odd")
        return {n: cams[n] for n in names}
    return {"front": C.look(e.pkg, s.root, W, H, dist=R.TWO_DIST), "yaw": C.look(e.pkg, s.root, W, H, dist=R.TWO_DIST, yaw=4.0),
            "gone": C.look(e.pkg, s.root, W, H, yaw=75.0)}


def _call(e, scene, b12, W, H, tiling=None, rows=None, stream=0, lib=None):
    """One batch call into patterned buffers -> (float bytes, RGB8 bytes, 8 counters)."""
    import torch
    F, rows = len(b12), H if rows is None else rows
    n = 3 * F * rows * W
    with torch.cuda.stream(stream) if stream else torch.cuda.stream(torch.cuda.current_stream()):
        px = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rgb = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        scene.render_batch_device(b12, np.repeat(e.sun[None], F, 0), W, H, mode=e.full, tiling=tiling, d_pixels=px.data_ptr(),
                                  d_rgb8=rgb.data_ptr(), d_counters=cnt.data_ptr(),
                                  stream=torch.cuda.current_stream().cuda_stream if stream else 0)
    return px, rgb, cnt, n


def _finish(px, rgb, cnt, n, F):
    import torch
    torch.cuda.synchronize()
    px, rgb = px.cpu().numpy(), rgb.cpu().numpy()
    assert (px[4 * n:] == 0xA5).all() and (rgb[n:] == 0xA5).all(), "a store behind the buffers"
    return px[:4 * n].reshape(F, -1), rgb[:n].reshape(F, -1), [int(x) for x in cnt.cpu().numpy()]


def _ref(e, s, key, b, W, H, tiling=None, rows=None):
    """The stats scene's one-frame launch of a view: computed once, shared, never changed."""
    if key not in s.refs:
        px, rgb, c = _finish(*_call(e, s.ref, b[None], W, H, tiling, rows), 1)
        px.setflags(write=False)
        rgb.setflags(write=False)
        s.refs[key] = (px[0], rgb[0], c[:4])
    return s.refs[key]


def _parity(e, s, views, W, H, tag=""):
    b12 = np.stack(list(views.values()))
    px, rgb, c = _finish(*_call(e, s.prod, b12, W, H), len(b12))
    assert c[6] == 0, "the launch's error word"
    want = [0, 0, 0, 0]
    for f, (v, b) in enumerate(views.items()):
        rp, rr, rc = _ref(e, s, (tag, v, W, H), b, W, H)
        assert np.array_equal(px[f], rp), f"float framebuffer of frame {f} ({v}) differs"
        assert np.array_equal(rgb[f], rr), f"RGB8 body of frame {f} ({v}) differs"
        want = [x + y for x, y in zip(want, rc)]
    assert c[:4] == want
    return b12


def _model(e, s, b12, W, H, got):
    """The model's retired tiles and group flags for the launch the scene ran last."""
    cut = s.prod.entry_nodes()["cut"]
    ret, rects = R.retired_tiles(e.pkg, cut, b12, s.root, W, H)
    flags, keep = R.group_flags(got["source"], True, got["tpw"], rects, ret, W, H, got["deal"])
    return ret, rects, flags, keep


def _check_readback(e, s, b12, W, H, tpw, need_mixed=True):
    got = s.prod.compact_order()
    assert got is not None and got["tpw"] == tpw, "the launch took the plain grid"
    ret, rects, flags, keep = _model(e, s, b12, W, H, got)
    rb = s.prod.retire()
    assert rb is not None and (rb["W"], rb["H"]) == (W, H), "the launch retired nothing"
    assert np.array_equal(rb["live"], ~ret), "the live mask"
    tx = (W + 7) // 8
    if tx % 32:
        assert not (rb["words"][..., -1] >> np.uint32(tx % 32)).any(), "bits past the last tile column"
    assert got["groups"] == len(flags) and np.array_equal(rb["flags"], flags), "the group flags"
    # from the model: a flagged group, and a kept group that holds a retired tile beside a live one
    f, by, bx = C.decode(got["order"][:got["device_tiles"]], True, W, H)
    dead = ret[f, by, bx]
    pad = -len(dead) % tpw
    g = np.concatenate([dead, np.ones(pad, bool)]).reshape(-1, tpw)
    assert np.array_equal(g.all(1).astype(np.uint8), flags)
    assert flags.any(), "no flagged group"
    if need_mixed:
        assert (g.any(1) & ~g.all(1)).any(), "no mixed group"
    return ret, rects, flags


CASES = [("bunny", 136, 72, 4), ("bunny", 1024, 1024, 2), ("bunny", 1160, 904, 2), ("two", 136, 72, 4), ("two", 1024, 1024, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,tpw", CASES)
def test_batches_match_single_stats_frames_and_the_model(env, name, W, H, tpw):
    s = env.scenes[name]
    views = _views(env, s, name, W, H)
    b12 = _parity(env, s, views, W, H)
    ret, rects, flags = _check_readback(env, s, b12, W, H, tpw)
    if name == "two":
        assert R.between_rows(ret[0]), "no tile-row with a retired run between live tiles"
    # the recording kernels: same bytes and counts, same mask and flags, and no group left early --
    # every tile that is not root-culled records its entry word
    s.prod.entry_record(True)
    try:
        _parity(env, s, views, W, H)
        _check_readback(env, s, b12, W, H, tpw)
        entries = s.prod.entry_nodes()["entries"].reshape(ret.shape)
        culled = C.culled_tiles(rects, W, H)
        assert np.array_equal(entries == env.pkg.ENTRY_CULLED, culled)
        assert np.array_equal(entries == env.pkg.ENTRY_EMPTY, ret & ~culled)
    finally:
        s.prod.entry_record(False)


@pytest.mark.gpu
def test_the_mask_follows_refit_and_update(env):
    """The second patch moves up, then further: the retired set changes with the scene's boxes."""
    e, W, H = env, 136, 72
    s = e.scenes["two"]
    views = _views(e, s, "two", W, H)
    b12 = np.stack(list(views.values()))
    _parity(e, s, views, W, H)
    before = s.prod.retire()["live"].copy()
    half = len(s.mesh) // 2
    try:
        for step, dy in enumerate((1.5, 3.0)):
            tri = s.mesh.tri.copy()
            tri[half:, 1] += dy
            moved = e.pkg.Mesh(tri, s.mesh.norm)
            if step == 0:
                s.prod.refit(moved)
                s.ref.refit(moved)
            else:
                s.prod.update(moved, 1e9, arith=e.pkg.ARITH_FMA)
                s.ref.update(moved, 1e9, arith=e.pkg.ARITH_FMA)
            s.root = M.root_box(tri)
            _parity(e, s, views, W, H, tag=f"moved{step}")
            ret, _, _ = _check_readback(e, s, b12, W, H, 4, need_mixed=False)
            assert not np.array_equal(~ret, before), "the move did not change the retired set"
            before = ~ret
    finally:
        s.prod.refit(s.mesh)
        s.ref.refit(s.mesh)
        s.root = M.root_box(s.mesh.tri)


@pytest.mark.gpu
def test_keep_rectangles_flag_nothing_beyond_the_root_cull(env):
    """tri1 (a cut of fewer than two nodes) and a view from inside the box: every rectangle is keep."""
    e, W, H = env, 136, 72
    mesh, bvh, _ = e.pkg.prepare(configs.CONFIGS["tri1"], arith=e.pkg.ARITH_FMA)
    t = _scene_env(e.pkg, mesh, bvh)
    try:
        views = {"centre": C.look(e.pkg, t.root, W, H), "gone": C.look(e.pkg, t.root, W, H, yaw=75.0)}
        b12 = _parity(e, t, views, W, H)
        # (a root that is a leaf has no cut, and its launches do not cull at all: the plain grid)
        rb = t.prod.retire()
        if t.prod.compact_order() is None:
            assert rb is None
        elif rb is not None:
            rects = [M.cull_rect(b, t.root, W, H) for b in b12]
            assert np.array_equal(rb["live"], ~C.culled_tiles(rects, W, H)) and not rb["flags"].any()
    finally:
        t.prod.close()
        t.ref.close()
    s = e.scenes["bunny"]
    cams = C.cameras(e.pkg, s.root, W, H)
    views = {"inside": cams["inside"], "odd": cams["odd"]}
    b12 = _parity(e, s, views, W, H)
    rb = s.prod.retire()
    assert rb is not None and rb["live"][0].all(), "the frame seen from inside keeps every tile"
    ret, rects = R.retired_tiles(e.pkg, s.prod.entry_nodes()["cut"], b12, s.root, W, H)
    assert np.array_equal(rb["live"], ~ret)


@pytest.mark.gpu
def test_24_bit_stacks_and_tilings_do_not_retire(env):
    e, W, H = env, 136, 72
    s = e.scenes["bunny"]
    cams = C.cameras(e.pkg, s.root, W, H)
    b12 = np.stack([cams["odd"], cams["gone"], cams["centre"]])
    _finish(*_call(e, s.prod, b12, W, H), 3)
    assert s.prod.retire() is not None
    for tiling, rows in ((e.pkg.Tiling(16, 1, 2, 0), None), (e.pkg.Tiling(24, 1, 3, 1), 24)):
        rows = e.pkg.local_rows(H, tiling) if rows is None else rows
        _, _, c = _finish(*_call(e, s.prod, b12, W, H, tiling, rows), 3)
        assert c[6] == 0 and s.prod.retire() is None, "a row-block / band tiling retired tiles"
    mesh, bvh, _ = e.pkg.prepare(configs.CONFIGS["proc_300"], arith=e.pkg.ARITH_FMA)
    p = _scene_env(e.pkg, mesh, bvh)
    try:
        assert p.prod.stack_width() == 3, "proc_300 walks with 24-bit stacks"
        views = {"centre": C.look(e.pkg, p.root, W, H), "gone": C.look(e.pkg, p.root, W, H, yaw=75.0)}
        _parity(e, p, views, W, H)
        assert p.prod.retire() is None, "a 24-bit-stack launch retired tiles"
    finally:
        p.prod.close()
        p.ref.close()


@pytest.mark.gpu
def test_two_streams_read_their_own_buffers(env):
    import torch
    e, W, H = env, 136, 72
    s = e.scenes["two"]
    v = _views(e, s, "two", W, H)
    batches = [{"front": v["front"], "gone": v["gone"]}, {"yaw": v["yaw"], "front": v["front"], "gone": v["gone"]}]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    calls = [_call(e, s.prod, np.stack(list(b.values())), W, H, stream=st) for b, st in zip(batches, streams)]
    for b, call in zip(batches, calls):
        px, rgb, c = _finish(*call, len(b))
        assert c[6] == 0
        for f, (name, basis) in enumerate(b.items()):
            rp, rr, _ = _ref(e, s, ("", name, W, H), basis, W, H)
            assert np.array_equal(px[f], rp) and np.array_equal(rgb[f], rr), f"frame {f} ({name}) differs"
    # the latest launch's read-back is its own cameras'
    _check_readback(e, s, np.stack(list(batches[1].values())), W, H, 4)


@pytest.mark.gpu
def test_counting_build_stores_every_pixel_once(env):
    """The diagnostic build: 15 B per pixel (float + RGB8) whichever path writes it; error word 0."""
    import importlib.util
    import os
    import torch
    e, W, H = env, 136, 72
    pkgdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ceres-raytracer_amd")
    path = os.path.join(pkgdir, "variants", "libceres_hip_count.so")
    assert os.path.exists(path), "the diagnostic build is part of build() (make all)"
    spec = importlib.util.spec_from_file_location("ceres_count_build_r", os.path.join(pkgdir, "__init__.py"),
                                                  submodule_search_locations=[pkgdir])
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    cb.LIB_PATH = path
    cb.lib()
    s = e.scenes["two"]
    sc = cb.Scene(s.mesh, s.bvh)
    try:
        b12 = np.stack(list(_views(e, s, "two", W, H).values()))
        F = len(b12)
        cb.fetch_counters(0, reset=True)
        px, rgb, c = _finish(*_call(e, sc, b12, W, H), F)
        n = cb.fetch_counters(0, reset=True)
        assert sc.retire() is not None and sc.retire()["flags"].any()
        assert n["store_vector"] == 15 * F * W * H
        assert c[6] == 0
    finally:
        sc.close()
