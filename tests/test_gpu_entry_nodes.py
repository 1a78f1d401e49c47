"""Entry nodes on the GPU: batch launches that compact start a kept tile's primary walk at the LCA
of the cut nodes whose rectangle reaches the tile (render_hip.hip "Entry nodes", csrc/entry_cut.hpp).

Image parity as in test_gpu_tile_compact.py: every byte of the float framebuffer and of the RGB8 body
(pre-filled with 0xA5, 64 guard bytes behind each) and the ray / hit / primary / shadow counts of the
batch on the production scene equal the same frames one per launch on a CERES_SCENE_STATS scene, which
never culls, compacts or enters below the root; the error word is 0.  Every batch runs twice: with the
production kernels, and with the kernels that record each tile's entry record, which must be the host
entry points' answer for the same camera (ceres_entry_rects, ceres_entry_tiles)."""
import importlib.util
import os

import numpy as np
import pytest

import configs
import cull_fill_model as M
import tile_compact_model as C


class _Env:
    pass


def _make_env(pkg, name):
    e = _Env()
    e.pkg = pkg
    e.cfg = configs.CONFIGS[name]
    e.mesh, e.bvh, _ = pkg.prepare(e.cfg, arith=pkg.ARITH_FMA)
    e.prod, e.ref = pkg.Scene(e.mesh, e.bvh), pkg.Scene(e.mesh, e.bvh, stats=True)
    e.root = M.root_box(e.mesh.tri)
    e.sun = np.asarray(e.cfg["sun"], np.float32)
    e.full = pkg.MODE_FULL | pkg.MODE_FMA
    e.refs = {}
    return e


@pytest.fixture(scope="module")
def envs(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make_env(pkg, name)
        return made[name]
    yield get
    for e in made.values():
        e.prod.close()
        e.ref.close()


def _call(e, scene, b12, W, H, tiling=None, rows=None):
    """One batch call into patterned buffers -> (float bytes, RGB8 bytes, 8 counters); guards checked."""
    import torch
    F, rows = len(b12), H if rows is None else rows
    n = 3 * F * rows * W
    px = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    scene.render_batch_device(b12, np.repeat(e.sun[None], F, 0), W, H, mode=e.full, tiling=tiling, d_pixels=px.data_ptr(),
                              d_rgb8=rgb.data_ptr(), d_counters=cnt.data_ptr())
    torch.cuda.synchronize()
    px, rgb = px.cpu().numpy(), rgb.cpu().numpy()
    assert (px[4 * n:] == 0xA5).all() and (rgb[n:] == 0xA5).all(), "a store behind the buffers"
    return px[:4 * n].reshape(F, -1), rgb[:n].reshape(F, -1), [int(x) for x in cnt.cpu().numpy()]


def _ref(e, b, W, H, tiling=None, rows=None, key=None):
    """The stats scene's one-frame launch of a view: computed once, shared, never changed."""
    key = (b.tobytes(), W, H, key)
    if key not in e.refs:
        px, rgb, c = _call(e, e.ref, b[None], W, H, tiling, rows)
        px.setflags(write=False)
        rgb.setflags(write=False)
        e.refs[key] = (px[0], rgb[0], c[:4])
    return e.refs[key]


def _parity(e, scene, b12, W, H, tiling=None, rows=None, key=None):
    px, rgb, c = _call(e, scene, b12, W, H, tiling, rows)
    assert c[6] == 0, "the launch's error word"
    want = [0, 0, 0, 0]
    for f, b in enumerate(b12):
        rp, rr, rc = _ref(e, b, W, H, tiling, rows, key)
        assert np.array_equal(px[f], rp), f"float framebuffer of frame {f} differs"
        assert np.array_equal(rgb[f], rr), f"RGB8 body of frame {f} differs"
        want = [x + y for x, y in zip(want, rc)]
    assert c[:4] == want
    return px, rgb, c


def _check_readback(e, scene, b12, W, H, cut=None):
    """The launch's rectangles and every recorded tile's entry record against the host entry points;
    returns (tiles with an empty set, tiles entering below the root, recorded tiles) per frame."""
    pkg = e.pkg
    got = scene.entry_nodes()
    assert got["used"] and (got["W"], got["H"]) == (W, H)
    cut = got["cut"] if cut is None else cut
    tx, ty = (W + 7) // 8, (H + 7) // 8
    ent = got["entries"].reshape(len(b12), ty, tx)
    rects = [M.cull_rect(b, e.root, W, H) for b in b12]
    culled = C.culled_tiles(rects, W, H)
    out = []
    for f, b in enumerate(b12):
        want_r = pkg.entry_rects(cut, b, W, H)
        assert np.array_equal(got["rects"][f], want_r), f"frame {f}: the launch's rectangles are not the host's"
        want = pkg.entry_tiles(cut, want_r, W, H)
        seen = ent[f] != pkg.ENTRY_CULLED
        assert seen[~culled[f]].all(), f"frame {f}: a kept tile recorded nothing"
        assert np.array_equal(ent[f][seen], want[seen]), f"frame {f}: a tile started at another record than the host says"
        out.append((int((ent[f][seen] == pkg.ENTRY_EMPTY).sum()), int(((ent[f][seen] != 0) & (ent[f][seen] != pkg.ENTRY_EMPTY)).sum()),
                    int(seen.sum())))
    return out


def _both(e, b12, W, H):
    """The batch with the recording kernels (read back) and with the production kernels."""
    e.prod.entry_record(True)
    try:
        _parity(e, e.prod, b12, W, H)
        stats = _check_readback(e, e.prod, b12, W, H)
    finally:
        e.prod.entry_record(False)
    _parity(e, e.prod, b12, W, H)
    got = e.prod.entry_nodes()
    assert got["used"] and len(got["entries"]) == 0
    return stats


def _views(e, W, H):
    return {"centre": C.look(e.pkg, e.root, W, H), "far": C.look(e.pkg, e.root, W, H, dist=4.0),
            "side": C.look(e.pkg, e.root, W, H, yaw=9.0, pitch=-4.0, dist=2.5), "gone": C.look(e.pkg, e.root, W, H, yaw=60.0),
            "inside": C.look(e.pkg, e.root, W, H, eye=C.scene_frame(e.root)[0])}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny_640", "dragon_333x217"])
@pytest.mark.parametrize("W,H,tpw", [(333, 217, 4), (136, 72, 4), (640, 480, 4)])
def test_batches_enter_below_the_root_and_match_single_stats_frames(envs, name, W, H, tpw):
    e = envs(name)
    v = _views(e, W, H)
    stats = _both(e, np.stack([v["centre"], v["side"], v["far"]]), W, H)
    assert e.prod.compact_order()["tpw"] == tpw
    assert sum(s[1] for s in stats) > 0, "no tile entered below the root"
    assert sum(s[0] for s in stats) > 0, "no kept tile had an empty set"


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,tpw", [(1920, 1080, 2), (2048, 2048, 4)])
def test_two_large_frames_take_the_two_tile_kernel_at_1080p_and_four_above(envs, W, H, tpw):
    e = envs("dragon_333x217")
    v = _views(e, W, H)
    stats = _both(e, np.stack([v["centre"], v["side"]]), W, H)
    assert e.prod.compact_order()["tpw"] == tpw
    assert sum(s[1] for s in stats) > 0 and sum(s[0] for s in stats) > 0


@pytest.mark.gpu
def test_one_batch_mixing_three_kinds_of_frame(envs):
    """Many empty-set tiles (the mesh small in the frame), the eye inside the root box (every
    rectangle "keep": the whole frame enters at the root) and a frame whose whole image misses."""
    e = envs("bunny_640")
    W, H = 333, 217
    v = _views(e, W, H)
    (empty, below, seen), inside, gone = _both(e, np.stack([v["far"], v["inside"], v["gone"]]), W, H)
    assert empty > 0 and below > 0
    assert inside == (0, 0, ((W + 7) // 8) * ((H + 7) // 8)), "the eye inside the box: every tile at the root"
    assert gone[:2] == (0, 0)


def _moved(pkg, mesh, root, shift):
    """The mesh with the half of its triangles right of the middle translated along x."""
    tri = mesh.tri.copy()
    cx = tri[:, 0] + (tri[:, 3] + tri[:, 6]) / 3
    tri[cx > 0.5 * (root[0] + root[1]), 0] += np.float32(shift)
    return pkg.Mesh(tri, mesh.norm)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["refit", "update"])
def test_refit_and_rebuild_refresh_the_cut(envs, how):
    """Half of proc_101 moved sideways by 0.3 scene diagonals (28 pixels at 136x72, more than three
    tiles): the batch of the refitted (or, through update, rebuilt) scene equals the batch of a fresh
    scene made from the moved triangles, and the read-back shows the boxes moved."""
    e = envs("proc_101")
    pkg = e.pkg
    W, H = 136, 72
    diag = C.scene_frame(e.root)[1]
    mesh2 = _moved(pkg, e.mesh, e.root, 0.3 * diag)
    root2 = M.root_box(mesh2.tri)
    b12 = np.stack([C.look(pkg, root2, W, H, dist=2.5), C.look(pkg, root2, W, H, yaw=6.0, dist=3.0)])
    scene = pkg.Scene(e.mesh, e.bvh)
    fresh = pkg.Scene(mesh2, pkg.build_bvh(mesh2, pkg.ARITH_FMA))
    try:
        before = scene.entry_nodes()["cut"]
        assert before.n == 64 and before.entry_ok == 1
        if how == "refit":
            scene.refit(mesh2)
        else:
            assert scene.update(mesh2, 1e-9, arith=pkg.ARITH_FMA)["rebuilt"] == 1
        after = scene.entry_nodes()["cut"]
        assert after.n == 64 and after.entry_ok == 1
        assert not np.array_equal(before.box, after.box), "the cut's boxes did not move"
        if how == "refit":
            assert np.array_equal(before.src, after.src) and np.array_equal(before.lca, after.lca), "a refit keeps the topology"
            pairs = scene.read_boxes()[0]
            assert np.array_equal(after.box, pairs.reshape(-1, 2, 6)[after.src >> 1, after.src & 1]), "the boxes are the refitted pairs'"
        want = _call(e, fresh, b12, W, H)
        e2 = _Env()
        e2.pkg, e2.root = pkg, root2
        for record in (True, False):
            scene.entry_record(record)
            got = _call(e, scene, b12, W, H)
            assert got[2][6] == 0 and got[2][:4] == want[2][:4]
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            if record:
                stats = _check_readback(e2, scene, b12, W, H)
                assert sum(s[1] for s in stats) > 0, "no tile entered below the root"
    finally:
        scene.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tri1", "quad"])
def test_small_scenes_enter_at_the_root(envs, name):
    """A root that is a leaf has no cut and its launches do not cull; quad's cut is its two leaves,
    whose LCA is always the root's record."""
    e = envs(name)
    W, H = 136, 72
    v = _views(e, W, H)
    b12 = np.stack([v["centre"], v["far"], v["side"]])
    cut = e.prod.entry_nodes()["cut"]
    e.prod.entry_record(True)
    try:
        _parity(e, e.prod, b12, W, H)
        got = e.prod.entry_nodes()
        if name == "tri1":
            assert cut.n == 0 and not got["used"] and e.prod.compact_order() is None
        else:
            assert 2 <= cut.n < 64 and cut.entry_ok == 1
            stats = _check_readback(e, e.prod, b12, W, H)
            if name == "quad":
                assert all(s[1] == 0 for s in stats), "two leaves under the root: no record but the root's"
    finally:
        e.prod.entry_record(False)
    _parity(e, e.prod, b12, W, H)


@pytest.mark.gpu
def test_stats_scenes_and_tilings_enter_at_the_root(envs):
    e = envs("bunny_640")
    W, H = 136, 72
    v = _views(e, W, H)
    b12 = np.stack([v["centre"], v["far"], v["side"]])
    e.prod.entry_record(True)
    try:
        _parity(e, e.prod, b12, W, H)
        assert e.prod.entry_nodes()["used"]
        for rank in (0, 1):
            t = e.pkg.Tiling(16, rank, 2, 0)
            _parity(e, e.prod, b12, W, H, tiling=t, rows=e.pkg.local_rows(H, t), key=("rb", rank))
            assert not e.prod.entry_nodes()["used"] and e.prod.compact_order() is None
    finally:
        e.prod.entry_record(False)
    e.ref.entry_record(True)
    try:
        _call(e, e.ref, b12, W, H)
        assert not e.ref.entry_nodes()["used"], "a stats scene keeps every ray's own root step"
    finally:
        e.ref.entry_record(False)


@pytest.mark.gpu
def test_counting_build_guard_stays_clear(envs):
    """The diagnostic build (libceres_hip_count.so, the stack guard compiled in): a compacting batch
    that enters below the root leaves the error word 0 and renders the product's bytes."""
    e = envs("dragon_333x217")
    pkgdir = os.path.dirname(e.pkg.__file__)
    path = os.path.join(pkgdir, "variants", "libceres_hip_count.so")
    assert os.path.exists(path), "the diagnostic build is part of build() (make all)"
    spec = importlib.util.spec_from_file_location("ceres_count_build_entry", os.path.join(pkgdir, "__init__.py"),
                                                  submodule_search_locations=[pkgdir])
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    cb.LIB_PATH = path
    cb.lib()
    W, H = 333, 217
    v = _views(e, W, H)
    b12 = np.stack([v["centre"], v["side"], v["far"]])
    sc = cb.Scene(e.mesh, e.bvh)
    try:
        _parity(e, sc, b12, W, H)
        assert sc.entry_nodes()["used"] and sc.compact_order() is not None
    finally:
        sc.close()
