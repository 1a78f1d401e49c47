"""Non-finite triangle soups (tests/soup_common.py) through the GPU builder and the device scene's upkeep:
ceres_bvh_build_device, ceres_scene_create_device, refit, rebuild, update, the SAH cost and the entry cut
on NaN, +-inf, 3e38-sized and denormal coordinates -- what a caller's simulation hands over when it blows up.

The GPU builder must make the host builder's tree, which tests/test_soups_cpu.py pins to the reference's own
(tests/golden/soups/soups.json); a device scene must answer like the host-made Scene and the CpuScene over
the host tree, and render the reference's frame.  The vacuity guards (frames with hits, culled tiles, tiles
entering below the root) are decided on the host, with CpuScene and the host entry points, before anything
is sent to the GPU.  Each test creates its scenes and runs them once."""
import functools
import hashlib
import math

import numpy as np
import pytest

import cull_fill_model as M
import entry_common as E
import quality_common as qc
import refit_common as rc
import soup_common as sc
import test_gpu_entry_nodes as EN
import test_gpu_refit as R
import test_soups_cpu as CPU
import trace_common as tc

pytestmark = pytest.mark.gpu

W, H = sc.FRAME_W, sc.FRAME_H
BW, BH = 136, 72
RENDERED_IDS = ["%s-%d" % c for c in sc.RENDERED]
FIX = CPU.FIX
bits = CPU.bits


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


# --------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("kind,n", sc.CASES, ids=sc.IDS)
def test_gpu_builder_equals_the_host_builder_and_the_reference(gpu, kind, n):
    """build_bvh_gpu against build_bvh in both arithmetics: node count, prim order, canonical sha256 --
    and the reference's own sha256.  A NaN bound of a primitive box must not reach the root box (k_init's
    keyed reduction) nor a bin of a small subtree (k_small's)."""
    pkg = gpu
    mesh = sc.mesh_of(pkg, kind, n)
    for arith in (0, 1):
        want = FIX["soups"]["%s-%d" % (kind, n)][CPU.BUILD[arith]]
        host = pkg.build_bvh(mesh, arith=arith)
        dev = pkg.build_bvh_gpu(mesh, arith=arith)
        print(kind, n, arith, "root host", host.nodes[0, :6].view(np.float32), "gpu", dev.nodes[0, :6].view(np.float32),
              "nodes", host.nodes.shape[0], dev.nodes.shape[0])
        assert dev.nodes.shape == host.nodes.shape, arith
        assert np.array_equal(dev.prim, host.prim), arith
        assert CPU.canon(dev) == CPU.canon(host), arith
        assert dev.nodes.shape[0] == want["n_nodes"] and CPU.canon(dev) == want["bvh_canonical_sha256"], arith


# --------------------------------------------------------------------------------------- scenes
def to_device(mesh):
    import torch
    return (torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0"), torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0"))


def device_scene(pkg, mesh, arith=0, stats=False):
    """Scene.from_device over build_bvh_device's tree of `mesh` (tensors returned to keep them alive)."""
    import torch
    n = len(mesh)
    d_tri, d_norm = to_device(mesh)
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream, arith)
    scene = pkg.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stats=stats, stream=stream)
    return scene, (d_tri, d_norm, d_nodes, d_prim)


def pose(pkg, kind, n, arith=0):
    """(basis12, sun) of a soup's 97 x 61 frame: the fixture's basis bits where the reference rendered it,
    else the same camera (tile_compact_model.look on the finite part's box) through pkg.Camera."""
    name = "%s-%d" % (kind, n)
    if name in FIX["frames"]:
        return CPU.frame_pose(name, arith)
    box = sc.finite_box(sc.soup(kind, n)[0])
    eye, d, up, fov = sc.frame_camera(box)
    return pkg.Camera(eye, d, up, fov, arith=arith).basis(W, H), sc.sun_of(box)


def frame_answers(scene, basis, sun, mode=0):
    px, rgb, st = scene.render(basis, sun, W, H, mode=mode)
    prim, tuv, sh, _ = scene.records(basis, sun, W, H, mode=mode)
    return dict(px=px, rgb=rgb, rays=st["rays"], hits=st["hits"], prim=prim, tuv=tuv, sh=sh)


def assert_frames_equal(a, b, what=""):
    for k in ("px", "rgb", "prim", "tuv", "sh"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
    assert (a["rays"], a["hits"]) == (b["rays"], b["hits"]), what


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_device_scene_frames(gpu, kind, n, arith):
    """build_bvh_device -> Scene.from_device against the host-made Scene and the CpuScene over the host
    tree: a solo 97 x 61 frame, full and primary-only, fast and robust slabs -- float pixels, RGB8, rays /
    hits (all three) and the per-pixel records (both GPU scenes); where the reference rendered the soup,
    its PPM sha256 and counts."""
    pkg = gpu
    name = "%s-%d" % (kind, n)
    mesh = sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(mesh, arith=arith)
    basis, sun = pose(pkg, kind, n, arith)
    fma = pkg.MODE_FMA if arith else 0
    modes = {"full": fma, "primary": fma | pkg.MODE_PRIMARY, "robust": fma | pkg.MODE_ROBUST,
             "robust-primary": fma | pkg.MODE_ROBUST | pkg.MODE_PRIMARY}
    cpu = pkg.CpuScene(mesh, bvh)
    try:
        want = {k: cpu.render(basis, sun, W, H, mode=m) for k, m in modes.items()}
    finally:
        cpu.close()
    for k, (_, _, st) in want.items():
        assert st["hits"] > 0, (k, "an empty frame checks nothing")
    host = pkg.Scene(mesh, bvh)
    dev, keep = device_scene(pkg, mesh, arith)
    try:
        a = {k: frame_answers(host, basis, sun, m) for k, m in modes.items()}
        b = {k: frame_answers(dev, basis, sun, m) for k, m in modes.items()}
    finally:
        host.close()
        dev.close()
    del keep
    for k in modes:
        px, rgb, st = want[k]
        print(name, k, st["rays"], st["hits"], b[k]["rays"], b[k]["hits"])
        assert_frames_equal(b[k], a[k], k)
        assert np.array_equal(bits(b[k]["px"]), bits(px)) and np.array_equal(b[k]["rgb"], rgb), k
        assert (b[k]["rays"], b[k]["hits"]) == (st["rays"], st["hits"]), k
        if name in FIX["frames"] and k in FIX["frames"][name][CPU.BUILD[arith]]:
            f = FIX["frames"][name][CPU.BUILD[arith]][k]
            assert (b[k]["rays"], b[k]["hits"]) == (f["rays"], f["hits"]), k
            assert hashlib.sha256(pkg.ppm(W, H, b[k]["rgb"])).hexdigest() == f["ppm_sha256"], k


def batch_env(pkg, mesh, bvh, prod, ref):
    e = EN._Env()
    e.pkg, e.mesh, e.bvh, e.prod, e.ref = pkg, mesh, bvh, prod, ref
    e.root = sc.root_of(bvh)                                           # what the launches cull with
    e.sun = sc.sun_of(sc.finite_box(mesh.tri))
    e.full = pkg.MODE_FULL | pkg.MODE_FMA
    e.refs = {}
    return e


@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_device_scene_batches(gpu, kind, n):
    """A 3-frame render_batch_device at 136 x 72 (views centre, side, far) into patterned buffers with guard
    bytes, against one-frame launches of a stats scene: every byte, the counts, error word 0; the recorded
    entries are the host entry points' answer.  `mixed` and `huge` are one leaf: their launches neither cull
    nor enter below the root, asserted instead."""
    pkg = gpu
    mesh = sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(mesh, pkg.ARITH_FMA)
    b12 = sc.views(pkg, sc.finite_box(mesh.tri), BW, BH)
    g = CPU.guard(kind, n)
    one_leaf = g["cut"] is None
    if one_leaf:                                                       # the guards, on the host, before the GPU sees anything
        assert kind in ("mixed", "huge") and all(g["keep"]) and bvh.nodes[0, 6] == n
    else:
        assert g["culled"] > 0 and g["cut"].entry_ok == 1 and (g["below"] > 0 or kind == "nan_p0")
    prod, keep = device_scene(pkg, mesh, pkg.ARITH_FMA)
    ref = pkg.Scene(mesh, bvh, stats=True)
    try:
        e = batch_env(pkg, mesh, bvh, prod, ref)
        cut = prod.entry_nodes()["cut"]
        if one_leaf:
            assert cut.n == 0
            prod.entry_record(True)
            EN._parity(e, prod, b12, BW, BH)
            assert not prod.entry_nodes()["used"] and prod.compact_order() is None
            prod.entry_record(False)
            EN._parity(e, prod, b12, BW, BH)
            return
        assert cut.entry_ok == 1 and cut.n == g["cut"].n
        stats = EN._both(e, b12, BW, BH)
        print(kind, n, "culled", g["culled"], "below the root: host", g["below"], "recorded", sum(s[1] for s in stats))
        assert (sum(s[1] for s in stats) > 0) == (g["below"] > 0) and (g["below"] > 0 or kind == "nan_p0")
        assert sum(s[2] for s in stats) >= 3 * ((BW + 7) // 8) * ((BH + 7) // 8) - g["culled"]
    finally:
        prod.close()
        ref.close()
    del keep


def soup_rays(pkg, kind, n):
    basis, _ = pose(pkg, kind, n)
    return np.concatenate([pkg.camera_rays(basis, W, H), tc.adversarial_rays()])


def queries(scene, rays, sun, mode):
    hits, occ, tst = scene.trace(rays, mode=mode, closest=True, occluded=True)
    spx, srgb, shits, status, sst = scene.shade(rays, sun, mode=mode, pixels=True, rgb8=True, hits=True, status=True)
    return dict(hits=hits, occ=occ, spx=spx, srgb=srgb, shits=shits, status=status,
                counts=(tst["rays"], tst["hits"], sst["rays"], sst["hits"]))


def assert_queries_equal(a, b, what=""):
    for k in ("hits", "occ", "spx", "srgb", "shits", "status"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
    assert a["counts"] == b["counts"], what


@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_ray_queries_equal_the_cpu_scene(gpu, kind, n):
    """Scene.trace (closest, occluded) and Scene.shade of a device scene on the frame's camera rays plus
    trace_common.adversarial_rays(), fast and robust: byte-equal to CpuScene over the host tree."""
    pkg = gpu
    mesh = sc.mesh_of(pkg, kind, n)
    rays = soup_rays(pkg, kind, n)
    _, sun = pose(pkg, kind, n)
    cpu = pkg.CpuScene(mesh, pkg.build_bvh(mesh))
    try:
        want = {m: queries(cpu, rays, sun, m) for m in (0, pkg.MODE_ROBUST)}
    finally:
        cpu.close()
    assert want[0]["counts"][1] > 0
    dev, keep = device_scene(pkg, mesh)
    try:
        got = {m: queries(dev, rays, sun, m) for m in (0, pkg.MODE_ROBUST)}
    finally:
        dev.close()
    del keep
    for m in got:
        assert_queries_equal(got[m], want[m], m)


# --------------------------------------------------------------------------------------- refit
def batch(pkg, scene, b12, sun):
    e = EN._Env()
    e.sun, e.full = sun, pkg.MODE_FULL | pkg.MODE_FMA
    return EN._call(e, scene, b12, BW, BH)


def recorded_batch(pkg, scene, b12, sun, root):
    """One batch with the recording kernels: error word 0, and -- where the launch entered at cut nodes --
    its rectangles and every tile's entry record are the host entry points' answer for the scene's own
    cut under `root`, the box the launch culls with.  Returns whether entries were used."""
    e = EN._Env()
    e.pkg, e.root, e.sun, e.full = pkg, root, sun, pkg.MODE_FULL | pkg.MODE_FMA
    scene.entry_record(True)
    try:
        out = EN._call(e, scene, b12, BW, BH)
        assert out[2][6] == 0, "the launch's error word"
        used = scene.entry_nodes()["used"]
        with np.errstate(all="ignore"):
            keep = [M.cull_rect(b, root, BW, BH) == M.KEEP for b in b12]
        if scene.entry_nodes()["cut"].n:                               # the eye inside an infinite or +-3e38 root: every
            assert used == (not all(keep))                             # rectangle "keep", nothing to compact or enter below
        if used:
            EN._check_readback(e, scene, b12, BW, BH)
    finally:
        scene.entry_record(False)
    return used


def cut_fields(scene):
    """The scene's cut table by field (bytes), for scene-against-scene equality."""
    cut = scene.entry_nodes()["cut"]
    return dict(n=cut.n, entry_ok=cut.entry_ok, src=cut.src.tobytes(), child=cut.child.tobytes(), box=cut.box.tobytes(),
                lca=cut.lca[:cut.n, :cut.n].tobytes(), depth=cut.depth[:cut.n, :cut.n].tobytes())


TOPOLOGY = ("n", "src", "child", "lca", "depth")    # what a refit keeps of a cut: it is chosen by box area at creation,
                                                    # and a refit reloads only its boxes (entry_cut.hpp, cut_load_box)


def check_scene_cut(pkg, scene, mesh, bvh):
    """A host-created scene's cut table passes entry_common.check_cut on the host layout's pair tree (the
    scene numbers its records like ceres_entry_relayout), and its boxes are the scene's pair boxes."""
    cut = scene.entry_nodes()["cut"]
    if bvh.nodes[0, 6]:
        assert cut.n == 0
        return cut
    pairs, _, _ = pkg.entry_relayout(mesh, bvh)
    E.check_cut(E.Tree(pairs, len(mesh)), cut)
    boxes = scene.read_boxes()[0]
    assert np.array_equal(bits(cut.box), bits(boxes.reshape(-1, 2, 6)[cut.src >> 1, cut.src & 1]))
    return cut


REFITS = [(k, n, how) for k in ("mixed", "mixed_nan", "nan_p0", "huge") for n in (300, 4097) for how in ("host", "device")]


@pytest.mark.parametrize("kind,n,how", REFITS, ids=["%s-%d-%s" % c for c in REFITS])
def test_refit_to_a_poisoned_soup_and_back(gpu, kind, n, how):
    """A scene of the finite base soup, refit / refit_device to the poisoned soup: pair boxes, frame,
    records, queries and a 3-frame batch equal a fresh scene's over refit_common.refit_nodes' tree (no box
    holds a NaN), the cut table is sound; refitted back to the base soup, the boxes and answers are those of
    a fresh scene over the base soup's refitted tree and the picture is the original scene's -- nothing
    stale."""
    pkg = gpu
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(base)
    moved = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, mesh.tri), bvh.prim)
    tight = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, base.tri), bvh.prim)
    basis, sun = pose(pkg, kind, n)
    b12 = sc.views(pkg, sc.finite_box(mesh.tri), BW, BH)
    rays = pkg.camera_rays(basis, W, H)
    keep = None
    if how == "host":
        s = pkg.Scene(base, bvh)
    else:
        s, keep = device_scene(pkg, base)
    fresh, fresh_back = pkg.Scene(mesh, moved), pkg.Scene(base, tight)
    try:
        before = frame_answers(s, basis, sun)
        assert before["hits"] > 0
        cut0 = cut_fields(s)
        batch(pkg, s, b12, sun)                                        # the old root box and cut have been in use

        def refit(m):
            if how == "host":
                s.refit(m)
            else:
                d_tri, d_norm = to_device(m)
                s.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
            tree = moved if m is mesh else tight
            return dict(frame=frame_answers(s, basis, sun), q=queries(s, rays, sun, 0), boxes=s.read_boxes(),
                        batch=batch(pkg, s, b12, sun), cost=(s.sah_cost(), s.sah_cost()),
                        used=recorded_batch(pkg, s, b12, sun, sc.root_of(tree)), cut=cut_fields(s),
                        cut_box=s.entry_nodes()["cut"].box.copy())

        def answers(f):
            return dict(frame=frame_answers(f, basis, sun), q=queries(f, rays, sun, 0), boxes=f.read_boxes(),
                        batch=batch(pkg, f, b12, sun), cost=(f.sah_cost(),), cut=cut_fields(f))

        got = refit(mesh)
        if how == "host":
            check_scene_cut(pkg, s, mesh, moved)
        back = refit(base)
        if how == "host":
            check_scene_cut(pkg, s, base, tight)
        want, want_back = answers(fresh), answers(fresh_back)
    finally:
        s.close()
        fresh.close()
        fresh_back.close()
    del keep
    for a, b, tree, what in ((got, want, moved, "poisoned"), (back, want_back, tight, "back")):
        assert_frames_equal(a["frame"], b["frame"], what)
        assert_queries_equal(a["q"], b["q"], what)
        assert a["batch"][2][6] == 0 and a["batch"][2][:4] == b["batch"][2][:4], what
        assert np.array_equal(a["batch"][0], b["batch"][0]) and np.array_equal(a["batch"][1], b["batch"][1]), what
        pairs, fp = a["boxes"][0], b["boxes"][0]
        assert not np.isnan(pairs).any() and not np.isnan(a["boxes"][1]).any(), what
        R.check_nodes4(a["boxes"][1], rc.box_set(tree.nodes), what)   # BVH4 child boxes: refitted BVH2 boxes
        print(kind, n, how, what, "entries used", a["used"], "cut", a["cut"]["n"], a["cut"]["entry_ok"])
        assert a["used"] == (what == "back" or kind in ("mixed_nan", "nan_p0")), what   # a finite root: the cut was used and read back
        assert a["cut"]["n"] == 64 and a["cut"]["entry_ok"] == 1, what
        assert all(a["cut"][k] == cut0[k] for k in TOPOLOGY), what     # the cut's nodes stay, their boxes are the tree's
        assert not np.isnan(a["cut_box"]).any() and {tuple(float(x) for x in r) for r in a["cut_box"]} <= rc.box_set(tree.nodes), what
        if how == "host":
            assert pairs.shape == fp.shape and np.array_equal(pairs, fp), what
            assert qc.dbits(a["cost"][0]) == qc.dbits(b["cost"][0]), what
        else:
            boxes = rc.box_set(tree.nodes)
            assert {tuple(float(x) for x in r[:6]) for r in pairs} | {tuple(float(x) for x in r[6:]) for r in pairs} <= boxes, what
        assert qc.dbits(a["cost"][0]) == qc.dbits(a["cost"][1]), what
    for k in ("px", "rgb", "prim", "tuv", "sh"):
        assert np.array_equal(bits(back["frame"][k]), bits(before[k])), k


# --------------------------------------------------------------------------------------- rebuild, update
def everything(pkg, scene, basis, sun, rays):
    pairs, nodes4 = scene.read_boxes()
    return dict(frame=frame_answers(scene, basis, sun), q=queries(scene, rays, sun, 0), info=scene.info(), pairs=pairs,
                nodes4=nodes4, cost=scene.sah_cost(), cut=cut_fields(scene))


def assert_everything_equal(a, b):
    assert_frames_equal(a["frame"], b["frame"])
    assert_queries_equal(a["q"], b["q"])
    assert a["info"] == b["info"]
    assert a["pairs"].shape == b["pairs"].shape and np.array_equal(bits(a["pairs"]), bits(b["pairs"]))
    assert (a["nodes4"] is None) == (b["nodes4"] is None)
    if a["nodes4"] is not None:
        assert a["nodes4"].shape == b["nodes4"].shape and np.array_equal(bits(a["nodes4"]), bits(b["nodes4"]))
    assert qc.dbits(a["cost"]) == qc.dbits(b["cost"])
    assert a["cut"] == b["cut"]                                       # src, child, box, lca, depth: the same cut


@functools.lru_cache(maxsize=None)
def fresh_device(kind, n):
    """Everything of ceres_scene_create_device over the GPU-built tree of the poisoned soup, computed once."""
    from conftest import import_package
    pkg = import_package()
    mesh = sc.mesh_of(pkg, kind, n)
    basis, sun = pose(pkg, kind, n)
    s, keep = device_scene(pkg, mesh)
    try:
        return everything(pkg, s, basis, sun, pkg.camera_rays(basis, W, H))
    finally:
        s.close()
        del keep


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_rebuild_to_a_poisoned_soup_equals_a_fresh_device_scene(gpu, kind, n, how):
    """rebuild (host arrays) / rebuild_device of a base-soup scene to the poisoned soup: frame, records,
    queries, info(), the box readback and the cost are ceres_scene_create_device's, bit for bit; the recorded
    entries of a batch are the host entry points' answer for the scene's own cut."""
    pkg = gpu
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, kind, n)
    basis, sun = pose(pkg, kind, n)
    s = pkg.Scene(base, pkg.build_bvh(base))
    try:
        if how == "host":
            s.rebuild(mesh)
        else:
            d_tri, d_norm = to_device(mesh)
            s.rebuild_device(d_tri.data_ptr(), d_norm.data_ptr())
        got = everything(pkg, s, basis, sun, pkg.camera_rays(basis, W, H))
        host_bvh = pkg.build_bvh(mesh)
        cut = s.entry_nodes()["cut"]
        if host_bvh.nodes[0, 6]:
            assert cut.n == 0
        else:
            assert cut.entry_ok == 1 and not np.isnan(cut.box).any()
            e = batch_env(pkg, mesh, host_bvh, s, None)
            b12 = sc.views(pkg, sc.finite_box(mesh.tri), BW, BH)
            s.entry_record(True)
            out = EN._call(e, s, b12, BW, BH)
            assert out[2][6] == 0
            EN._check_readback(e, s, b12, BW, BH)
            s.entry_record(False)
    finally:
        s.close()
    assert_everything_equal(got, fresh_device(kind, n))


def same_cost(a, b, n_nodes):
    """Two evaluations of the cost definition: both NaN, the same infinity, or within quality_common's
    relative bound (n + 16) * 2^-52 of each other."""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= (n_nodes + 16) * 2.0 ** -52 * abs(b)


@pytest.mark.parametrize("ratio", [1e-9, 2.0, math.inf])
@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_update_decides_like_the_cpu_scene(gpu, kind, n, ratio):
    """update(poisoned, max_ratio) on a base-soup scene: the same rebuilt / kept decision and the same cost
    fields as CpuScene.update (a NaN cost never rebuilds), and the scene that results: the fresh device
    scene when rebuilt, the refitted one when kept."""
    pkg = gpu
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(base)
    basis, sun = pose(pkg, kind, n)
    cpu = pkg.CpuScene(base, bvh)
    try:
        want = cpu.update(mesh, ratio)
    finally:
        cpu.close()
    s = pkg.Scene(base, bvh)
    kept = None
    try:
        cut0 = cut_fields(s)
        u = s.update(mesh, ratio)
        got = frame_answers(s, basis, sun)
        cut = cut_fields(s)
        b12 = sc.views(pkg, sc.finite_box(mesh.tri), BW, BH)
        if not u["rebuilt"]:
            moved = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, mesh.tri), bvh.prim)
            check_scene_cut(pkg, s, mesh, moved)                       # the kept tree's refreshed cut
            if kind == "huge":                                         # finite boxes that overflow in float only: the model holds
                qc.assert_cost(u["cost"], moved.nodes, "refitted to huge")
            used = recorded_batch(pkg, s, b12, sun, sc.root_of(moved))
            f = pkg.Scene(mesh, moved)
            try:
                kept = frame_answers(f, basis, sun)
                assert all(cut[k] == cut0[k] for k in TOPOLOGY)
            finally:
                f.close()
        else:
            used = recorded_batch(pkg, s, b12, sun, sc.root_of(pkg.build_bvh(mesh)))
            assert cut == fresh_device(kind, n)["cut"]
        print(kind, n, ratio, "entries used", used)
    finally:
        s.close()
    print(kind, n, ratio, u, want)
    assert u["rebuilt"] == want["rebuilt"]
    m = bvh.nodes.shape[0]
    assert same_cost(u["cost"], want["cost"], m) and same_cost(u["built_cost"], want["built_cost"], m)
    if u["rebuilt"]:                                                  # the new tree's cost: the fresh device scene's bits
        assert qc.dbits(u["new_cost"]) == qc.dbits(fresh_device(kind, n)["cost"])
    else:
        assert qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
    assert_frames_equal(got, fresh_device(kind, n)["frame"] if u["rebuilt"] else kept)


@functools.lru_cache(maxsize=None)
def fresh_base(n):
    """The frames and the cut of ceres_scene_create_device over the GPU-built tree of the finite base soup."""
    from conftest import import_package
    pkg = import_package()
    s, keep = device_scene(pkg, sc.base_mesh(pkg, n))
    try:
        return dict(frames={k: frame_answers(s, *pose(pkg, k, n)) for k, m in sc.RENDERED if m == n}, cut=cut_fields(s))
    finally:
        s.close()
        del keep


@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=RENDERED_IDS)
def test_update_back_to_the_finite_soup_rebuilds_like_the_cpu_scene(gpu, kind, n):
    """The other way round, which does rebuild: a scene BUILT over the poisoned soup (its cost is n for the
    one-leaf tree of `mixed`, and negative where a bin's empty +-FLT_MAX axis reached a node box) updated to
    the finite base soup with max_ratio 1e-9: the CPU scene's decision, and when rebuilt the fresh device
    scene of the base soup with its cost bits."""
    pkg = gpu
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(mesh)
    basis, sun = pose(pkg, kind, n)
    cpu = pkg.CpuScene(mesh, bvh)
    try:
        want = cpu.update(base, 1e-9)
    finally:
        cpu.close()
    s = pkg.Scene(mesh, bvh)
    try:
        u = s.update(base, 1e-9)
        got = frame_answers(s, basis, sun)
        cost = s.sah_cost()
        cut = cut_fields(s)
        used = recorded_batch(pkg, s, sc.views(pkg, sc.finite_box(base.tri), BW, BH), sun, sc.root_of(pkg.build_bvh(base)))
    finally:
        s.close()
    print(kind, n, u, want)
    assert u["rebuilt"] == want["rebuilt"] == 1
    assert same_cost(u["cost"], want["cost"], bvh.nodes.shape[0])
    assert qc.dbits(u["new_cost"]) == qc.dbits(cost) and same_cost(cost, want["new_cost"], 2 * n) and cost > 1.0
    assert_frames_equal(got, fresh_base(n)["frames"][kind])
    assert used and cut == fresh_base(n)["cut"]                       # the rebuilt tree's cut, used and read back
