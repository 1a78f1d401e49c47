"""Non-finite triangle soups (tests/soup_common.py) through the host builder and the CPU scene, against
the fixture the reference's own BinnedSahBuilder and render() recorded for the same bytes
(tests/golden/soups/soups.json, tests/golden/make_golden_soups.py).  No GPU needed.

The reference's answers these tests pin: bounding_box.hpp:23-27 extends with std::min / std::max, so a
NaN bound that arrives second is dropped -- by the per-primitive extend (a NaN p1 / p2), the root fold and
every bin fold -- while a box seeded from a NaN p0 keeps it; a NaN centre goes to bin 0; one infinite or
huge row makes the root's diagonal infinite and the whole tree one leaf."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest

import quality_common as qc
import refit_common as rc
import soup_common as sc

FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soups", "soups.json")))
BUILD = {0: "exact", 1: "ref"}
FRAME_IDS = ["%s-%d" % c for c in sc.FRAMES]
RENDERED_IDS = ["%s-%d" % c for c in sc.RENDERED]
W, H = sc.FRAME_W, sc.FRAME_H
FINITE_ROOT = ("nan_p0", "nan_p0_first", "nan_p0_last", "nan_edge", "mixed_nan")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def canon(bvh):
    import oracle
    return oracle.canonical_bvh_sha(bvh.nodes, bvh.prim)


def leaves(bvh):
    """(first, count) of every leaf reachable from the root."""
    out, stack = [], [0]
    while stack:
        k = stack.pop()
        cnt, first = int(bvh.nodes[k, 6]), int(bvh.nodes[k, 7])
        if cnt:
            out.append((first, cnt))
        else:
            stack += [first, first + 1]
    return out


def test_no_kind_was_dropped_and_every_case_is_recorded():
    assert FIX["dropped"] == {} and FIX["seed"] == sc.SEED
    assert sorted(FIX["soups"]) == sorted(sc.IDS) and sorted(FIX["frames"]) == sorted(FRAME_IDS)


@pytest.mark.parametrize("kind,n", sc.CASES, ids=sc.IDS)
def test_generator_is_pinned(kind, n):
    """The soup's bytes are the ones the reference was given; the poisoned share and what each kind promises."""
    tri, marked = sc.soup(kind, n)
    again, _ = sc.soup(kind, n)
    assert tri.tobytes() == again.tobytes() and sc.sha(tri) == FIX["soups"]["%s-%d" % (kind, n)]["tri48_sha256"]
    bad = sc.nonfinite_rows(tri)
    if kind in ("all_nan", "denormal"):
        assert marked.all()
    else:
        assert marked.sum() == sc.share(n) and (n < 16 or 10 * marked.sum() <= n)
        assert np.array_equal(tri[~marked], sc.base(n)[~marked]) and not bad[~marked].any()
    u = tri.view(np.uint32)
    if kind.startswith("nan_p0"):
        assert np.isnan(tri[marked, 0:3]).any(axis=1).all() and np.isfinite(tri[marked, 3:9]).all()
        assert kind != "nan_p0_first" or marked[0]
        assert kind != "nan_p0_last" or marked[n - 1]
        if marked.sum() >= 4:
            assert set(sc.NANS) <= set(u[marked, 0:3].reshape(-1).tolist())
    elif kind == "nan_edge":
        assert np.isfinite(tri[:, 0:3]).all() and np.isnan(tri[marked, 3:9]).any(axis=1).all()
    elif kind == "inf":
        assert np.isinf(tri[marked, 0:3]).any(axis=1).all() and not np.isnan(tri[:, :9]).any()
        with np.errstate(invalid="ignore"):
            assert np.isnan(tri[marked, 0:3] - tri[marked, 3:6]).any()            # inf - inf
    elif kind == "huge":
        m = tri[marked]
        v = np.stack([m[:, 0:3], m[:, 0:3] - m[:, 3:6], m[:, 0:3] + m[:, 6:9]], axis=1)
        assert np.isfinite(m[:, :9]).all() and np.isfinite(v).all() and not bad.any()     # vertices and edges finite
        assert (np.abs(m[:, 0:3]) == np.float32(3e38)).all() and (np.abs(v) > 2.69e38).all()
        with np.errstate(over="ignore"):
            assert np.isinf(v.max(axis=(0, 1)) - v.min(axis=(0, 1))).all()               # the root diagonal overflows
    elif kind == "denormal":
        assert (tri[:, 0:3] >= 1e-45).all() and (tri[:, 0:3] <= 1e-39).all() and not bad.any()
    elif kind == "all_nan":
        assert np.isnan(tri[:, 0:3]).all()
    elif kind == "mixed" and marked.sum() >= 6:
        m = tri[marked]
        assert np.isnan(m[:, 0:3]).any() and np.isnan(m[:, 3:9]).any() and np.isinf(m[:, 0:3]).any()
        assert (np.abs(m[:, 0:3]) == np.float32(3e38)).any() and ((m[:, 0:3] > 0) & (m[:, 0:3] < 1e-39)).any()
    elif kind == "mixed_nan" and marked.sum() >= 3:
        m = tri[marked]
        assert np.isnan(m[:, 0:3]).any() and np.isnan(m[:, 3:9]).any() and not np.isinf(m).any()


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("kind,n", sc.CASES, ids=sc.IDS)
def test_host_builder_equals_the_reference(pkg, kind, n, arith):
    """build_bvh makes the reference's tree: node count, canonical sha256; prim is a permutation and the
    leaves tile it, so every row -- the non-finite ones included -- sits in exactly one leaf."""
    want = FIX["soups"]["%s-%d" % (kind, n)][BUILD[arith]]
    bvh = pkg.build_bvh(sc.mesh_of(pkg, kind, n), arith=arith)
    assert bvh.nodes.shape[0] == want["n_nodes"]
    assert canon(bvh) == want["bvh_canonical_sha256"]
    assert sorted(bvh.prim.tolist()) == list(range(n))
    spans = sorted(leaves(bvh))
    assert spans[0][0] == 0 and all(a + c == b for (a, c), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) == n
    root = bvh.nodes[0, :6].view(np.float32)
    if kind in FINITE_ROOT:
        assert np.isfinite(root).all()
    elif kind == "all_nan":
        assert root.tolist() == [sc.FLT_MAX, -sc.FLT_MAX] * 3
    else:
        assert not np.isnan(root).any()
    if kind in ("inf", "huge", "denormal") or (kind == "mixed" and n >= 200):
        assert bvh.nodes.shape[0] == 1                    # the reference's one-leaf tree (see soup_common)


def frame_pose(name, arith):
    """(basis12, sun) of a fixture frame in a build's arithmetic: the reference's own basis bits."""
    f = FIX["frames"][name]
    bb = f[BUILD[arith]]["basis"]
    b = np.asarray([int(h, 16) for h in bb["dir"] + bb["u"] + bb["v"]], np.uint32).view(np.float32)
    return (np.concatenate([np.asarray([float(x) for x in f["eye"]], np.float32), b]),
            np.asarray([float(x) for x in f["sun"]], np.float32))


def frame_modes(pkg, arith):
    fma = pkg.MODE_FMA if arith else 0
    return {"full": pkg.MODE_FULL | fma, "primary": pkg.MODE_PRIMARY | fma, "robust": pkg.MODE_FULL | pkg.MODE_ROBUST | fma}


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("kind,n", sc.FRAMES, ids=FRAME_IDS)
def test_cpu_scene_renders_the_reference_frame(pkg, kind, n, arith):
    """CpuScene over the host BVH: the reference's PPM and ray / hit counts at 97 x 61, full, primary-only
    and with the robust node intersector.  The frames are not empty (the fixture's hits > 0)."""
    name = "%s-%d" % (kind, n)
    f = FIX["frames"][name]
    mesh = sc.mesh_of(pkg, kind, n)
    assert hashlib.sha256(mesh.norm.tobytes()).hexdigest() == f["norm36_sha256"]
    basis, sun = frame_pose(name, arith)
    s = pkg.CpuScene(mesh, pkg.build_bvh(mesh, arith=arith))
    try:
        for which, mode in frame_modes(pkg, arith).items():
            want = f[BUILD[arith]][which]
            _, rgb, st = s.render(basis, sun, W, H, mode=mode)
            print(name, which, st["rays"], st["hits"])
            assert want["hits"] > 0 and (st["rays"], st["hits"]) == (want["rays"], want["hits"]), which
            assert hashlib.sha256(pkg.ppm(W, H, rgb)).hexdigest() == want["ppm_sha256"], which
    finally:
        s.close()
    assert f[BUILD[arith]]["full"]["loop_vs_render_mismatch"] == 0


def cpu_answers(pkg, scene, basis, sun):
    px, rgb, st = scene.render(basis, sun, W, H)
    rays = pkg.camera_rays(basis, W, H)
    hits, occ, tst = scene.trace(rays, closest=True, occluded=True)
    keys = ("rays", "hits", "node_pairs", "tri_tests")
    return dict(px=px, rgb=rgb, hits=hits, occ=occ, st={k: st[k] for k in keys}, tst={k: tst[k] for k in keys})


def assert_same(a, b):
    for k in ("px", "rgb", "hits", "occ"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert a["st"] == b["st"] and a["tst"] == b["tst"]


REFITS = [(k, n) for k in ("mixed", "mixed_nan", "nan_p0", "nan_edge", "inf", "huge", "all_nan") for n in (300, 4097)]


@pytest.mark.parametrize("kind,n", REFITS, ids=["%s-%d" % c for c in REFITS])
def test_cpu_refit_to_a_poisoned_soup_and_back(pkg, kind, n):
    """CpuScene.refit from the finite base soup to its poisoned version: frame, traversal counters and
    trace equal a fresh CpuScene over refit_common.refit_nodes' restatement (std::min / std::max, no NaN in
    any box); the cost is the same bits twice.  Refitted back, nothing stale is left: pixels and hits are the
    original scene's, and the traversal counters those of a fresh scene over the base soup's refitted tree
    (a refit's boxes are tight, the builder's are unions of bins, so the counters of the BUILT tree differ)."""
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(base)
    moved = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, mesh.tri), bvh.prim)
    assert not np.isnan(rc.node_fields(moved.nodes)[0]).any()
    basis, sun = frame_pose(FRAME_IDS[0], 0)
    s, fresh = pkg.CpuScene(base, bvh), pkg.CpuScene(mesh, moved)
    tight = pkg.CpuScene(base, pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, base.tri), bvh.prim))
    try:
        before = cpu_answers(pkg, s, basis, sun)
        s.refit(mesh)
        got, want = cpu_answers(pkg, s, basis, sun), cpu_answers(pkg, fresh, basis, sun)
        cost = (s.sah_cost(), s.sah_cost(), fresh.sah_cost())
        s.refit(base)
        back, back_want = cpu_answers(pkg, s, basis, sun), cpu_answers(pkg, tight, basis, sun)
    finally:
        s.close()
        fresh.close()
        tight.close()
    assert_same(got, want)
    assert qc.dbits(cost[0]) == qc.dbits(cost[1]) == qc.dbits(cost[2])
    assert_same(back, back_want)
    for k in ("px", "rgb", "hits", "occ"):
        assert np.array_equal(bits(back[k]), bits(before[k])), k
    assert before["st"]["hits"] > 0


@pytest.mark.parametrize("kind,n", sc.RENDERED, ids=["%s-%d" % c for c in sc.RENDERED])
def test_cost_of_a_built_tree_is_the_same_bits_twice(pkg, kind, n):
    mesh = sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(mesh)
    s = pkg.CpuScene(mesh, bvh)
    try:
        a, b = s.sah_cost(), s.sah_cost()
    finally:
        s.close()
    print(kind, n, a)
    assert qc.dbits(a) == qc.dbits(b)
    if bvh.nodes[0, 6]:
        assert a == float(n)                                          # a root leaf costs its triangle count


@pytest.mark.parametrize("ratio", [1e-9, 2.0, math.inf])
@pytest.mark.parametrize("n", [300, 4097])
def test_update_with_a_nan_cost_does_not_rebuild(pkg, n, ratio):
    """Refitted to `mixed`, boxes are infinite and the cost is inf / inf: `cost > max_ratio * built_cost` is
    false for a NaN, so update keeps the tree however small max_ratio is -- and the scene is the refitted one."""
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, "mixed", n)
    bvh = pkg.build_bvh(base)
    moved = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, mesh.tri), bvh.prim)
    basis, sun = frame_pose(FRAME_IDS[0], 0)
    s, fresh = pkg.CpuScene(base, bvh), pkg.CpuScene(mesh, moved)
    try:
        u = s.update(mesh, ratio)
        got, want = cpu_answers(pkg, s, basis, sun), cpu_answers(pkg, fresh, basis, sun)
    finally:
        s.close()
        fresh.close()
    assert math.isnan(u["cost"]) and math.isnan(u["new_cost"]) and u["rebuilt"] == 0 and np.isfinite(u["built_cost"])
    assert_same(got, want)


@functools.lru_cache(maxsize=None)
def guard(kind, n):
    from conftest import import_package
    pkg = import_package()
    mesh = sc.mesh_of(pkg, kind, n)
    bvh = pkg.build_bvh(mesh, pkg.ARITH_FMA)
    return sc.batch_guard(pkg, mesh, bvh, sc.views(pkg, sc.finite_box(mesh.tri), 136, 72), 136, 72)


def test_the_gpu_batches_are_not_vacuous():
    """What test_gpu_soups.py's 136 x 72 batches rely on, decided on the host: `mixed_nan` 4097 has culled
    tiles and tiles entering below the root; `nan_p0` 300 has culled tiles (its 64 cut boxes of long
    triangles all reach every kept tile: nothing enters below the root); `mixed` 4097 is one leaf under an
    infinite root and `huge` 4097 one leaf under a root of +-3e38 that holds the eye, so they have no cut and
    every frame's rectangle is "keep" -- asserted instead."""
    for kind, n in (("mixed_nan", 4097), ("nan_p0", 300)):
        g = guard(kind, n)
        print(kind, n, "culled", g["culled"], "below", g["below"], "cut", g["cut"].n, g["cut"].entry_ok)
        assert g["cut"].entry_ok == 1 and g["culled"] > 0 and (g["below"] > 0) == (kind == "mixed_nan"), (kind, n)
    for kind in ("mixed", "huge"):                        # one leaf under an infinite / a +-3e38 root box
        g = guard(kind, 4097)
        print(kind, g["rects"])
        assert g["cut"] is None and all(g["keep"]), kind


@pytest.mark.parametrize("kind,n", [c for c in sc.RENDERED if c[0] != "mixed"], ids=[i for i in RENDERED_IDS if not i.startswith("mixed-")])
@pytest.mark.parametrize("refit", [False, True], ids=["built", "refitted"])
def test_the_cut_of_a_poisoned_tree_is_sound(pkg, kind, n, refit):
    """ceres_entry_cut_build on the host layout of a poisoned soup's tree -- as built, with NaN bounds in
    boxes seeded from a NaN p0, and as refitted from the base soup's tree, with inverted infinite axes --
    passes entry_common.check_cut: every root-to-leaf path meets the cut once, depth-first order, LCAs."""
    import entry_common as E
    mesh = sc.mesh_of(pkg, kind, n)
    if refit:
        b = pkg.build_bvh(sc.base_mesh(pkg, n))
        bvh = pkg.Bvh(rc.refit_nodes(b.nodes, b.prim, mesh.tri), b.prim)
    else:
        bvh = pkg.build_bvh(mesh)
    pairs, _, rlc = pkg.entry_relayout(mesh, bvh)
    if bvh.nodes[0, 6]:                                   # `huge` as built: one leaf, nothing to cut
        assert kind == "huge" and not refit and rlc == n
        return
    cut = pkg.entry_cut(pairs, rlc, sc.root_of(bvh))
    assert rlc == 0 and cut.n == 64
    E.check_cut(E.Tree(pairs, n), cut)


@pytest.mark.parametrize("n", [300, 4097])
def test_cost_of_a_refit_to_huge_matches_the_model(pkg, n):
    """Refitted to `huge`, every box is finite but up to 6e38 wide: hi - lo overflows in float, not in the
    cost's doubles.  The cost is finite and matches quality_common's numpy model within its bound (every
    term is non-negative); it FALLS, because it is relative to the root's half area, so update at
    max_ratio 2 keeps the tree."""
    base, mesh = sc.base_mesh(pkg, n), sc.mesh_of(pkg, "huge", n)
    bvh = pkg.build_bvh(base)
    moved = pkg.Bvh(rc.refit_nodes(bvh.nodes, bvh.prim, mesh.tri), bvh.prim)
    with np.errstate(over="ignore"):
        b = rc.node_fields(moved.nodes)[0]
        assert np.isfinite(b).all() and np.isinf(b[:, 1::2] - b[:, 0::2]).any()
    s = pkg.CpuScene(base, bvh)
    try:
        u = s.update(mesh, 2.0)
    finally:
        s.close()
    print(n, u)
    qc.assert_cost(u["cost"], moved.nodes, "refitted to huge")
    qc.assert_cost(u["built_cost"], bvh.nodes, "as built")
    assert u["rebuilt"] == 0 and u["cost"] < u["built_cost"] and qc.dbits(u["new_cost"]) == qc.dbits(u["cost"])
