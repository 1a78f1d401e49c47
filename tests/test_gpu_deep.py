"""Render, query and upkeep paths on scenes whose BVH is 52 to 64 levels deep (tests/deep_common.py).

Code sized or switched by depth that no shallower scene reaches: the unclamped BVH2 walk under its
bound stack_entries = depth; the stealing loop's first-passing-child bound and ordered records once
40 or more 16-bit entries cost waves (arms6: nearest-first 61 against 26); the wave-wide shadow
packet's fallback to the per-lane loop when the bound passes its 64 lanes (bodyarms, device-built:
67); the query kernels' LDS sized by the nearest-first bound; the level-by-level device layout and
refit; the GPU builder's small-subtree stack at the depth cap; the primary-only kernel's LDS at 64
levels (cap26).  Every comparison is bitwise: with the reference's fixtures (frames, counts,
records), with CpuScene, or with a fresh device scene.

The first thing this module does with a mesh is to create its CERES_SCENE_STATS scene and render
with it: the stats kernels clamp every stack access and report an overflow as an error, so a bound
too small for these trees shows there as CERES_ESTACK and not as a store past the stack.  The frames
of the arms6_* / bodyarms_* configs are also rendered by every suite parametrised over the fixtures
(solo frames, the GPU builder and OBJ parser, the ray sets arms6_centroids / bodyarms_centroids of
test_gpu_trace.py and test_gpu_trace_scenes.py, the double scenes of test_gpu_f64.py)."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, load_ref_records

import configs
import cull_fill_model as M
import deep_common as dc
import refit_common as rc
import tile_compact_model as C
import trace_common as tc
from test_gpu_shadow_stack import _bounds
from test_gpu_stack_widths import forced
import test_gpu_entry_nodes as EN
import test_gpu_retire as RT

pytestmark = pytest.mark.gpu

ARITHS = [0, 1]
BUILD = {0: "exact", 1: "ref"}
MESH_CONFIGS = {m: [n for n in configs.DEEP if n.startswith(m + "_")] for m in ("arms6", "bodyarms")}


def _groups(mesh):
    """A mesh's configs by (mode, robust, W, H): the frames one batch launch can hold."""
    out = {}
    for n in MESH_CONFIGS[mesh]:
        c = configs.CONFIGS[n]
        out.setdefault((c["mode"], c["robust"], c["W"], c["H"]), []).append(n)
    return out


class _Env:
    """One mesh: its Tri48 / BVH in both arithmetics and its scenes by (arith, kind)."""

    def __init__(self, pkg, name, obj):
        self.pkg, self.name = pkg, name
        self.prep = {}
        for a in ARITHS:
            mesh = pkg.load_obj(obj, a)
            self.prep[a] = (mesh, pkg.build_bvh(mesh, a))
        self.scenes, self.keep, self.built = {}, [], {}
        # the clamped walks first: a full and a primary-only frame of every arithmetic
        for a in ARITHS:
            st = self.scene(a, "stats")
            b12, sun, W, H = self.any_view(a)
            fma = pkg.MODE_FMA if a else 0
            for mode in (pkg.MODE_FULL, pkg.MODE_PRIMARY, pkg.MODE_FULL | pkg.MODE_ROBUST):
                st.render(b12, sun, W, H, mode=mode | fma)

    def any_view(self, arith):
        if self.name == "cap26":
            cfg, e, b12, sun = cap26_view(self.pkg, "full", arith)
            return b12, sun, cfg["W"], cfg["H"]
        b12, sun, cfg = view_of(MESH_CONFIGS[self.name][0], arith)[:3]
        return b12, sun, cfg["W"], cfg["H"]

    def scene(self, arith, kind="host"):
        """kind: stats | host | device (GPU-built BVH, device relayout) | device_stats."""
        import torch
        pkg = self.pkg
        if (arith, kind) not in self.scenes:
            mesh, bvh = self.prep[arith]
            if kind in ("host", "stats"):
                sc = pkg.Scene(mesh, bvh, stats=kind == "stats")
            else:
                n = len(mesh)
                d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
                d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
                d_nodes = torch.empty((2 * n - 1) * 8, dtype=torch.int32, device="cuda:0")
                d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
                stream = torch.cuda.current_stream().cuda_stream
                m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream, arith)
                sc = pkg.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(),
                                           stats=kind == "device_stats", stream=stream)
                torch.cuda.synchronize()
                self.built[arith] = (d_nodes.cpu().numpy().view(np.uint32).reshape(-1, 8)[:m], d_prim.cpu().numpy().astype(np.uint64))
                self.keep += [d_tri, d_norm, d_nodes, d_prim]
            self.scenes[arith, kind] = sc
        return self.scenes[arith, kind]

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def envs(pkg, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Env(pkg, name, dc.obj_path(name, tmp_path_factory.mktemp(name)))
        return made[name]
    yield get
    for e in made.values():
        e.close()


def view_of(name, arith):
    """(basis12, sun, cfg, meta, records) of a deep config in one build, from the fixture's bits."""
    meta, rec, _ = load_golden(name)
    if arith:
        rec = load_ref_records(name)
    b, p = (meta["ref_basis"], meta["ref_pose"]) if arith else (meta["basis"], meta["pose"])
    b12 = np.concatenate([dc.bits(p["eye"]), dc.bits(b["dir"] + b["u"] + b["v"])]).astype(np.float32)
    return b12, dc.bits(p["sun"]), configs.CONFIGS[name], meta, rec


def cap26_view(pkg, view, arith):
    e = dc.load_cap26()["views"][view][BUILD[arith]]
    return dc.cap26_cfg(view, None), e, np.concatenate([dc.bits(e["eye"]), dc.bits(e["basis"])]).astype(np.float32), dc.bits(e["sun"])


def _check_px(px, rgb, st, W, H, pkg, sha, rays_hits, rec=None, what=""):
    assert hashlib.sha256(pkg.ppm(W, H, rgb)).hexdigest() == sha, what
    if st is not None:
        assert (st["rays"], st["hits"]) == rays_hits, what
    if rec is not None:
        pix = rec["pixel"].astype(np.int64)
        assert np.array_equal(np.asarray(px).view(np.uint32).reshape(-1, 3)[pix], rec["rgb"].view(np.uint32)), what


def _check_records(got, rec, full, what):
    prim, tuv, sh = got[:3]
    pix = rec["pixel"].astype(np.int64)
    hit = rec["prim"] >= 0
    assert np.array_equal(prim[pix], rec["prim"]), what
    if full:
        assert np.array_equal(sh[pix], rec["shadow"]), what
    for k, key in enumerate(("t", "u", "v")):
        assert np.array_equal(tuv[pix][hit, k].view(np.uint32), rec[key][hit].view(np.uint32)), (what, key)


def _batch(pkg, scene, b12, sun, W, H, mode):
    """One batch call -> (float [F, 3WH], RGB8 [F, 3WH], counters); guard bytes behind both buffers."""
    import torch
    F = len(b12)
    n = 3 * F * W * H
    px = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    scene.render_batch_device(b12, sun, W, H, mode=mode, d_pixels=px.data_ptr(), d_rgb8=rgb.data_ptr(), d_counters=cnt.data_ptr())
    torch.cuda.synchronize()
    px, rgb = px.cpu().numpy(), rgb.cpu().numpy()
    assert (px[4 * n:] == 0xA5).all() and (rgb[n:] == 0xA5).all(), "a store behind the buffers"
    c = [int(x) for x in cnt.cpu().numpy()]
    assert c[6] == 0, "the launch's error word"
    return px[:4 * n].view(np.float32).reshape(F, -1), rgb[:n].reshape(F, -1), c


# ---------------------------------------------------------------- 1. bounds

@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", ["arms6", "bodyarms", "cap26"])
def test_bounds_equal_the_restatement(envs, name, arith):
    """depth, stack_entries and both BVH4 bounds of host-made and device-built scenes; the host-made
    ones are ordered without being asked (their nearest-first stacks cost waves), the device-built
    ones keep build order: bodyarms and cap26 there carry a bound above the packet's 64 lanes."""
    e = envs(name)
    depth, _ = dc.depth_and_leaf(e.prep[arith][1].nodes)
    near, first = _bounds(e.prep[arith][1].nodes)
    for kind, want in (("stats", (near, first)), ("host", (near, first)), ("device", (near, near))):
        info = e.scene(arith, kind).info()
        assert (info["depth"], info["stack_entries"]) == (depth, depth), kind
        assert (info["shadow_stack_nearest"], info["shadow_stack_first"]) == want, kind
    assert e.scene(arith, "host").stack_width() == 2
    if name == "arms6":
        assert 40 <= depth <= 63 and near >= 2 * first and first <= 64
    else:
        assert near > 64 >= first and (name == "bodyarms" or depth == 64)


# ---------------------------------------------------------------- 2. frames and batches against the reference

@pytest.mark.parametrize("kind", ["stats", "host", "device"])
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", ["arms6", "bodyarms"])
def test_frames_and_batches_equal_the_reference(envs, name, arith, kind):
    """Every view: a solo frame (the stealing kernel) with its hit records, then 3- and 16-frame
    batches of the views that share a mode and a size -- PPM bytes, float pixels, rays and hits."""
    e = envs(name)
    pkg = e.pkg
    sc = e.scene(arith, kind)
    if kind == "device" and name == "bodyarms":
        assert sc.info()["shadow_stack_first"] > 64, "the batch below is the one that must leave the wave-wide packet"
    for (mode, robust, W, H), names in _groups(name).items():
        views = [view_of(n, arith) for n in names]
        m = pkg.cfg_mode(views[0][2], arith)
        for n, (b12, sun, cfg, meta, rec) in zip(names, views):
            b = BUILD[arith]
            px, rgb, st = sc.render(b12, sun, W, H, mode=m)
            _check_px(px, rgb, st, W, H, pkg, meta["ppm_sha256"][b], (meta[b]["rays"], meta[b]["hits"]), rec, (n, kind, "solo"))
            _check_records(sc.records(b12, sun, W, H, mode=m), rec, mode == "full", (n, kind))
        if kind == "stats":
            continue
        for F in (3, 16):
            pick = [views[f % len(views)] for f in range(F)]
            px, rgb, c = _batch(pkg, sc, np.stack([v[0] for v in pick]), np.stack([v[1] for v in pick]), W, H, m)
            for f, (b12, sun, cfg, meta, rec) in enumerate(pick):
                _check_px(px[f], rgb[f], None, W, H, pkg, meta["ppm_sha256"][BUILD[arith]], None, rec, (names, kind, F, f))
            assert c[0] == sum(v[3][BUILD[arith]]["rays"] for v in pick) and c[1] == sum(v[3][BUILD[arith]]["hits"] for v in pick)


# ---------------------------------------------------------------- 3. cull, compaction, entry nodes, retirement

class _Pair:
    pass


@pytest.mark.parametrize("W,H,tpw", [(136, 72, 4), (1024, 1024, 2)])
def test_cull_compaction_entry_nodes_and_retirement(envs, W, H, tpw):
    """tile_compact_model's cameras (odd / gone / centre / inside) on arms6: the production batch
    against one-frame launches of the stats scene, with the recorded entry nodes held to the host
    entry points and the live mask and group flags to tests/retire_model.py."""
    env = envs("arms6")
    pkg = env.pkg
    e = _Pair()
    e.pkg, e.full = pkg, pkg.MODE_FULL | pkg.MODE_FMA
    e.mesh, e.bvh = env.prep[1]
    e.prod, e.ref = env.scene(1, "host"), env.scene(1, "stats")
    e.root = M.root_box(e.mesh.tri)
    e.sun = dc.bits(load_golden("arms6_wide")[0]["ref_pose"]["sun"])
    e.refs = {}
    cams = C.cameras(pkg, e.root, W, H)
    views = {k: cams[k] for k in ("odd", "gone", "centre", "inside")}
    b12 = RT._parity(e, e, views, W, H)
    got = e.prod.compact_order()
    assert got is not None and got["tpw"] == tpw
    ret, rects, flags, keep = RT._model(e, e, b12, W, H, got)
    rb = e.prod.retire()
    assert rb is not None and np.array_equal(rb["live"], ~ret) and np.array_equal(rb["flags"], flags)
    print("arms6", W, H, "retired tiles", int(ret.sum()), "of", ret.size, "flagged groups", int(flags.sum()), "of", len(flags))
    e.prod.entry_record(True)
    try:
        RT._parity(e, e, views, W, H)
        stats = EN._check_readback(e, e.prod, b12, W, H)
    finally:
        e.prod.entry_record(False)
    print("arms6", W, H, "per frame (empty sets, below the root, recorded):", stats)
    assert sum(s[1] for s in stats) > 0, "no tile entered below the root"


# ---------------------------------------------------------------- 4. stack widths

@pytest.mark.parametrize("width", [3, 4])
def test_bodyarms_on_wider_stacks(envs, width):
    """CERES_DEBUG_STACK_WIDTH=3 and =4: the 24- and 32-bit stack kernels under a 53-level tree and a
    BVH4 bound of 67 -- a solo frame and a batch against the fixtures (reference-flag build)."""
    e = envs("bodyarms")
    pkg = e.pkg
    mesh, bvh = e.prep[1]
    with forced(width):
        sc = pkg.Scene(mesh, bvh)
    try:
        assert sc.stack_width() == width
        (mode, robust, W, H), names = next((k, v) for k, v in _groups("bodyarms").items() if len(v) > 1)
        views = [view_of(n, 1) for n in names]
        m = pkg.cfg_mode(views[0][2], 1)
        for n, (b12, sun, cfg, meta, rec) in zip(names, views):
            px, rgb, st = sc.render(b12, sun, W, H, mode=m)
            _check_px(px, rgb, st, W, H, pkg, meta["ppm_sha256"]["ref"], (meta["ref"]["rays"], meta["ref"]["hits"]), rec, (n, width))
        px, rgb, c = _batch(pkg, sc, np.stack([v[0] for v in views]), np.stack([v[1] for v in views]), W, H, m)
        for f, (b12, sun, cfg, meta, rec) in enumerate(views):
            _check_px(px[f], rgb[f], None, W, H, pkg, meta["ppm_sha256"]["ref"], None, rec, (names[f], width, "batch"))
    finally:
        sc.close()


# ---------------------------------------------------------------- 5. ray queries

def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name", ["arms6", "bodyarms"])
def test_queries_equal_the_cpu_path(envs, name, kind):
    """The centroid rays (trace_common.centroid_rays; their closest-hit and occlusion answers are held to
    the reference's by the ray-set suites): trace and shade of the GPU scene against CpuScene, fast and
    robust, both arithmetics, and the device-pointer entry points against the host calls."""
    import torch
    e = envs(name)
    pkg = e.pkg
    rays = tc.centroid_rays(name + "_centroids")
    n = len(rays)
    for arith in ARITHS:
        sc = e.scene(arith, kind)
        cpu = pkg.CpuScene(*e.prep[arith])
        sun = view_of(MESH_CONFIGS[name][0], arith)[1]
        try:
            for robust in (0, pkg.MODE_ROBUST):
                mode = (pkg.MODE_FMA if arith else 0) | robust
                h, o, st = sc.trace(rays, mode=mode, closest=True, occluded=True)
                hc, oc, stc = cpu.trace(rays, mode=mode, closest=True, occluded=True)
                assert h.tobytes() == hc.tobytes() and np.array_equal(o, oc), (arith, robust)
                assert (st["rays"], st["hits"]) == (stc["rays"], stc["hits"])
                assert (h["prim"] >= 0).any() and (h["prim"] < 0).any()
                a = sc.shade(rays, sun, mode=mode, pixels=True, rgb8=True, hits=True, status=True)
                b = cpu.shade(rays, sun, mode=mode, pixels=True, rgb8=True, hits=True, status=True)
                for x, y, what in zip(a[:4], b[:4], ("pixels", "rgb8", "hits", "status")):
                    assert np.array_equal(_raw(x), _raw(y)), (arith, robust, what)
                assert set(np.unique(a[3])) == {0, 1, 2}, "misses, lit and shadowed rays"
                # the device-pointer entry points
                d_rays = torch.from_numpy(np.array(rays)).cuda()
                d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
                d_occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
                stream = torch.cuda.current_stream().cuda_stream
                sc.trace_device(d_rays.data_ptr(), n, mode=mode, d_hits16=d_hits.data_ptr(), d_occluded=d_occ.data_ptr(), stream=stream)
                d_px = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
                sc.shade_device(d_rays.data_ptr(), n, sun, mode=mode, d_pixels=d_px.data_ptr(), d_status=d_st.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                assert d_hits.cpu().numpy().tobytes() == h.tobytes() and np.array_equal(d_occ.cpu().numpy(), o)
                assert np.array_equal(_raw(d_px.cpu().numpy()), _raw(a[0])) and np.array_equal(d_st.cpu().numpy(), a[3])
        finally:
            cpu.close()


# ---------------------------------------------------------------- 6. double scenes

@pytest.mark.parametrize("arith", ARITHS)
def test_double_scene_queries_equal_the_cpu_path(envs, arith):
    """arms6 in double (its frames against the reference's render<double>: tests/golden/f64/arms6_*,
    test_gpu_f64.py): the double builder's tree is as deep, and trace_rays_f64 / shade_rays_f64 on the
    centroid rays equal CpuScene's answers."""
    e = envs("arms6")                                               # (the float stats scene has rendered)
    pkg = e.pkg
    cfg = configs.CONFIGS["arms6_zoom20"]
    mesh, bvh, _ = pkg.prepare(cfg, f64=True, arith=arith)
    depth = dc.depth_and_leaf(bvh.nodes)[0]
    assert depth >= 40
    rays = tc.centroid_rays("arms6_centroids").astype(np.float64)
    sun = np.asarray(pkg.pose_f64(cfg, arith)[1], np.float64)
    sc, cpu = pkg.Scene(mesh, bvh), pkg.CpuScene(mesh, bvh)
    try:
        assert sc.info()["depth"] == depth
        mode = pkg.MODE_FMA if arith else 0
        h, o, st = sc.trace(rays, mode=mode, closest=True, occluded=True)
        hc, oc, stc = cpu.trace(rays, mode=mode, closest=True, occluded=True)
        assert h.tobytes() == hc.tobytes() and np.array_equal(o, oc)
        assert (h["prim"] >= 0).any() and (h["prim"] < 0).any()
        a = sc.shade(rays, sun, mode=mode, pixels=True, rgb8=True, hits=True, status=True)
        b = cpu.shade(rays, sun, mode=mode, pixels=True, rgb8=True, hits=True, status=True)
        for x, y, what in zip(a[:4], b[:4], ("pixels", "rgb8", "hits", "status")):
            assert np.array_equal(_raw(x), _raw(y)), what
    finally:
        sc.close()
        cpu.close()


# ---------------------------------------------------------------- 7. upkeep

@pytest.mark.parametrize("how", ["refit", "rebuild", "update_keeps", "update_rebuilds"])
@pytest.mark.parametrize("name", ["arms6", "bodyarms", "cap26"])
def test_upkeep_equals_fresh_scenes(envs, name, how):
    """Every arm scaled by its own power of two (deep_common.moved), reference-flag arithmetic: the
    scene after refit / rebuild / update against CpuScene over the numpy-refitted or the host-rebuilt
    BVH and against a fresh device scene of it -- sah_cost, a solo frame and a 3-frame batch."""
    import math
    import quality_common as qc
    e = envs(name)
    pkg = e.pkg
    mesh, bvh = e.prep[1]
    moved = dc.moved(pkg, mesh, name)
    cfg = configs.CONFIGS["arms6_zoom20"] if name != "cap26" else dc.cap26_cfg("full", None)
    cam, sun = pkg.pose(cfg, arith=1)
    W, H, mode = cfg["W"], cfg["H"], pkg.cfg_mode(cfg, 1)
    b12 = np.asarray(cam.basis(W, H), np.float32)
    keeps = how in ("refit", "update_keeps")
    new_bvh = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim) if keeps else pkg.build_bvh(moved, 1)
    cpu, fresh, sc = pkg.CpuScene(moved, new_bvh), pkg.Scene(moved, new_bvh), pkg.Scene(mesh, bvh)
    try:
        if how == "refit":
            sc.refit(moved)
        elif how == "rebuild":
            sc.rebuild(moved, arith=1)
        elif how == "update_keeps":
            assert sc.update(moved, math.inf, arith=1)["rebuilt"] == 0
        else:
            assert sc.update(moved, 1e-9, arith=1)["rebuilt"] == 1
        assert sc.info()["depth"] == dc.depth_and_leaf(new_bvh.nodes)[0] >= 40
        qc.assert_cost(sc.sah_cost(), new_bvh.nodes, how)
        want = cpu.render(b12, sun, W, H, mode=mode)
        assert 10 * want[2]["hits"] >= W * H
        for s, what in ((sc, how), (fresh, "fresh")):
            px, rgb, st = s.render(b12, sun, W, H, mode=mode)
            assert np.array_equal(_raw(px), _raw(want[0])) and np.array_equal(rgb, want[1]), what
            assert (st["rays"], st["hits"]) == (want[2]["rays"], want[2]["hits"]), what
            bpx, brgb, c = _batch(pkg, s, np.repeat(b12[None], 3, 0), np.repeat(np.asarray(sun, np.float32)[None], 3, 0), W, H, mode)
            for f in range(3):
                assert np.array_equal(_raw(bpx[f]), _raw(want[0])) and np.array_equal(brgb[f], want[1]), (what, f)
    finally:
        for s in (cpu, fresh, sc):
            s.close()


# ---------------------------------------------------------------- 8. cap26: the depth cap

@pytest.mark.parametrize("arith", ARITHS)
def test_cap26_gpu_builder_matches_the_reference(envs, arith):
    """64 levels through the GPU builder (k_small's work stack at the cap) and the device relayout."""
    import oracle
    e = envs("cap26")
    e.scene(arith, "device")
    nodes, prim = e.built[arith]
    want = dc.load_cap26()["scene_" + BUILD[arith]]
    assert len(nodes) == want["n_nodes"]
    assert oracle.canonical_bvh_sha(np.ascontiguousarray(nodes).reshape(-1), prim) == want["bvh_canonical_sha256"]


@pytest.mark.parametrize("kind", ["stats", "host", "device"])
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("view", ["full", "zoom"])
def test_cap26_full_mode_equals_the_reference(envs, view, arith, kind):
    from test_deep_cpu import check_cap26_frame, check_cap26_records
    e = envs("cap26")
    pkg = e.pkg
    sc = e.scene(arith, kind)
    cfg, ent, b12, sun = cap26_view(pkg, view, arith)
    W, H, mode = cfg["W"], cfg["H"], pkg.cfg_mode(cfg, arith)
    check_cap26_frame(pkg, sc, view, arith)
    prim, tuv, sh = sc.records(b12, sun, W, H, mode=mode)[:3]
    check_cap26_records(pkg, view, arith, prim, tuv, sh)
    if kind != "stats":
        for F in (3, 16):
            px, rgb, c = _batch(pkg, sc, np.repeat(b12[None], F, 0), np.repeat(sun[None], F, 0), W, H, mode)
            for f in range(F):
                assert hashlib.sha256(pkg.ppm(W, H, rgb[f])).hexdigest() == ent["ppm_sha256"], (F, f)
            assert (c[0], c[1]) == (F * ent["rays"], F * ent["hits"])


@pytest.mark.parametrize("kind", ["stats", "host", "device"])
@pytest.mark.parametrize("arith", ARITHS)
def test_cap26_primary_only_frame(envs, arith, kind):
    """MODE_PRIMARY at 64 levels.  The primary-only kernel's 256-lane workgroups and 4-byte entries need
    (64 + 1) x 256 x 4 = 66,560 B of LDS at the depth cap, its largest launch; that is more than 64 KB
    but well inside the 160 KB a gfx950 workgroup may take (hipDeviceProp_t::sharedMemPerBlock, which the
    launch checks), so the frame renders: it, its records and a 3-frame batch are the reference's
    primary-only frame, and the robust one the CPU path's."""
    import torch
    from test_deep_cpu import check_cap26_frame, check_cap26_records
    e = envs("cap26")
    pkg = e.pkg
    sc = e.scene(arith, kind)
    assert sc.info()["depth"] == 64
    lds = getattr(torch.cuda.get_device_properties(0), "shared_memory_per_block", None)
    print("sharedMemPerBlock", lds)
    assert lds is None or lds >= 65 * 256 * 4
    cfg, ent, b12, sun = cap26_view(pkg, "primary", arith)
    W, H, mode = cfg["W"], cfg["H"], pkg.cfg_mode(cfg, arith)
    px, rgb = check_cap26_frame(pkg, sc, "primary", arith)
    cpu = pkg.CpuScene(*e.prep[arith])                              # the robust slabs: no reference frame, the CPU path's
    try:
        want = cpu.render(b12, sun, W, H, mode=mode | pkg.MODE_ROBUST)
    finally:
        cpu.close()
    got = sc.render(b12, sun, W, H, mode=mode | pkg.MODE_ROBUST)
    assert np.array_equal(_raw(got[0]), _raw(want[0])) and np.array_equal(got[1], want[1]) and got[2]["hits"] == want[2]["hits"]
    prim, tuv, sh = sc.records(b12, sun, W, H, mode=mode)[:3]
    check_cap26_records(pkg, "primary", arith, prim, tuv, None)
    if kind != "stats":
        bpx, brgb, c = _batch(pkg, sc, np.repeat(b12[None], 3, 0), np.repeat(sun[None], 3, 0), W, H, mode)
        for f in range(3):
            assert np.array_equal(brgb[f], rgb) and np.array_equal(_raw(bpx[f]), _raw(px)), f


@pytest.mark.parametrize("width", [3, 4])
def test_cap26_on_wider_stacks(envs, width):
    """64 levels under CERES_DEBUG_STACK_WIDTH=3 and =4 (65 slots of 3 and 4 bytes per lane): the
    full-mode frames and the primary-only frame are the reference's."""
    from test_deep_cpu import check_cap26_frame
    e = envs("cap26")
    pkg = e.pkg
    mesh, bvh = e.prep[1]
    with forced(width):
        sc = pkg.Scene(mesh, bvh)
    try:
        assert sc.stack_width() == width
        for view in ("full", "zoom", "primary"):
            check_cap26_frame(pkg, sc, view, 1)
    finally:
        sc.close()
