"""Entry nodes on the host (csrc/entry_cut.hpp through ceres_entry_*; no GPU): the cut table of a pair
array, the rectangles of a camera and the record a tile's primary walk starts at.

Cut and table: every root-to-leaf path meets the cut exactly once, the cut is in depth-first order,
lca[i][j] is a brute-force LCA, and a child box poking out of its parent clears entry_ok.
Tiles against the oracle (FMA arithmetic, want_records): for every pixel with a primary hit, the cut
node above the hit triangle's leaf has a rectangle that reaches the pixel's tile, the tile's entry
record is an ancestor-or-self of the record holding that leaf, and no tile with a hit is empty --
without exception.  Degenerate cameras enter at the root everywhere."""
import numpy as np
import pytest

import configs
import entry_common as E

_cache = {}


def _scene(pkg, name):
    """(cfg, tree, cut, index of cut src -> number, orig slot of every original triangle), shared and never changed."""
    if name not in _cache:
        cfg = configs.CONFIGS[name]
        mesh, bvh, _ = pkg.prepare(cfg, arith=pkg.ARITH_FMA)
        pairs, orig, rlc = pkg.entry_relayout(mesh, bvh)
        root = bvh.nodes[0, :6].copy().view(np.float32)
        cut = pkg.entry_cut(pairs, rlc, root)
        tree = E.Tree(pairs, len(mesh))
        slot_of = np.empty(len(mesh), np.int64)
        slot_of[orig] = np.arange(len(mesh))
        _cache[name] = (cfg, tree, cut, rlc, slot_of, root)
    return _cache[name]


@pytest.mark.parametrize("name", ["dragon_333x217", "bunny_640", "proc_101", "dupleaf", "tri1", "quad"])
def test_cut_and_lca_table(pkg, name):
    cfg, tree, cut, rlc, _, _ = _scene(pkg, name)
    if name == "tri1":
        assert rlc and cut.n == 0 and cut.entry_ok == 0, "a root that is a leaf has no cut"
        return
    assert not rlc
    n_inner = len(tree.pairs)
    assert cut.n == min(64, n_inner + 1), "expanded until 64 nodes or no inner node is left"
    assert cut.entry_ok == 1
    E.check_cut(tree, cut)
    if name == "quad":
        assert cut.n == 2 and (cut.child == E.LEAF).all() and (cut.lca[:2, :2] == 0).all()


def _hand_tree(poke):
    """Root -> (inner A, leaf), A -> (leaf, leaf); poke: A's right child reaches past A by one ulp."""
    def rec(lb, rb, lc, lf, rc, rf):
        r = np.zeros(16, np.uint32)
        r[:6] = np.asarray(lb, np.float32).view(np.uint32)
        r[6:12] = np.asarray(rb, np.float32).view(np.uint32)
        r[12:] = [lc, lf, rc, rf]
        return r
    hi = np.nextafter(np.float32(1), np.float32(2)) if poke else np.float32(1)
    p0 = rec([0, 1, 0, 1, 0, 1], [2, 3, 0, 1, 0, 1], 0, 1, 1, 2)
    p1 = rec([0, 0.5, 0, 1, 0, 1], [0.5, hi, 0, 1, 0, 1], 1, 0, 1, 1)
    return np.stack([p0, p1]), np.asarray([0, 3, 0, 1, 0, 1], np.float32)


def test_a_child_box_poking_out_of_its_parent_clears_entry_ok(pkg):
    pairs, root = _hand_tree(False)
    cut = pkg.entry_cut(pairs, 0, root)
    assert cut.n == 3 and cut.entry_ok == 1
    assert [int(x) for x in cut.src] == [2, 3, 1], "depth-first: A's children, then the root's right child"
    E.check_cut(E.Tree(pairs, 3), cut)
    pairs, root = _hand_tree(True)
    cut = pkg.entry_cut(pairs, 0, root)
    assert cut.n == 3 and cut.entry_ok == 0
    # ... and then every rectangle is "keep": every tile enters at the root
    b = np.asarray([0.5, 0.5, -5, 0, 0, 1, 0.01, 0, 0, 0, 0.01, 0], np.float32)
    rects = pkg.entry_rects(cut, b, 64, 48)
    assert (rects == [0, 0xffff, 0, 0xffff]).all()
    assert (pkg.entry_tiles(cut, rects, 64, 48) == 0).all()


def _check_view(pkg, name, cfg, sc, basis9, eye, sun):
    import oracle
    _, tree, cut, _, slot_of, _ = _scene(pkg, name)
    index = {int(s): k for k, s in enumerate(cut.src)}
    W, H = cfg["W"], cfg["H"]
    ref = oracle.render(sc, cfg, basis=basis9, eye=eye, sun=sun, want_records=True, want_ppm=False, want_pixels=False)
    b12 = np.concatenate([np.asarray(eye, np.float32), np.asarray(basis9, np.float32)])
    rects = pkg.entry_rects(cut, b12, W, H)
    tiles = pkg.entry_tiles(cut, rects, W, H)
    reach = E.tile_sets(rects, W, H)
    # the host entry point against the rectangles themselves
    any_k = reach.any(2)
    lo, hi = reach.argmax(2), 63 - reach[:, :, ::-1].argmax(2)
    assert np.array_equal(tiles, np.where(any_k, cut.lca[lo, hi], pkg.ENTRY_EMPTY))
    prim = ref["prim"].reshape(H, W)                                 # row j = the ray of v = 2 (j + 0.5) / H - 1
    jj, ii = np.nonzero(prim >= 0)
    assert len(jj), "the view hits nothing"
    leaf = tree.leaf_of_slot[slot_of[prim[jj, ii]]]
    assert (leaf >= 0).all()
    combos = np.unique(np.stack([jj // 8, ii // 8, leaf], 1), axis=0)
    above = {}
    for ty, tx, lf in combos:
        k = above.setdefault(int(lf), E.cut_above(tree, index, int(lf)))
        assert tiles[ty, tx] != pkg.ENTRY_EMPTY, f"tile ({tx}, {ty}) has a hit and no cut rectangle"
        assert reach[ty, tx, k], f"tile ({tx}, {ty}): the cut node above a hit leaf is not in S"
        assert int(tiles[ty, tx]) in tree.record_ancestors(int(lf) >> 1), f"tile ({tx}, {ty}) enters beside a hit leaf"
    return int((~any_k).sum()), int((tiles != 0).sum())


@pytest.mark.parametrize("name", ["dragon_333x217", "dragon_orbit3_333x217", "bunny_orbit7_160x120", "bunny_97x61_primary"])
def test_tiles_are_consistent_with_the_oracle(pkg, name):
    import oracle
    cfg = dict(configs.CONFIGS[name], mode="full")
    sc = oracle.prepare(cfg, contract=True)
    empty, below = _check_view(pkg, name, cfg, sc, sc["basis"], sc["eye"], sc["sun"])
    assert below > 0, "no tile enters below the root: the check would be vacuous"


def test_sixteen_orbit_views_of_the_dragon(pkg):
    import oracle
    cfg = dict(configs.CONFIGS["dragon_333x217"], W=160, H=120)
    sc = oracle.prepare(cfg, contract=True)
    below = 0
    for f in range(16):
        eye, dir, sun = (sc["eye"], np.asarray(cfg["dir"], np.float32), sc["sun"]) if f == 0 else \
            oracle.orbit(configs.BENCH_AXIS, 22.5, f, cfg["eye"], cfg["dir"], cfg["sun"], True)
        basis = oracle.camera_basis(eye, dir, cfg["up"], cfg["fov"], cfg["W"], cfg["H"], True)
        below += _check_view(pkg, "dragon_333x217", cfg, sc, basis, eye, sun)[1]
    assert below > 0


def test_degenerate_cameras_enter_at_the_root(pkg):
    cfg, tree, cut, _, _, root = _scene(pkg, "dragon_333x217")
    W, H = 160, 120
    cam = pkg.Camera(cfg["eye"], cfg["dir"], cfg["up"], cfg["fov"], arith=pkg.ARITH_FMA)
    good = cam.basis(W, H)
    assert (pkg.entry_tiles(cut, pkg.entry_rects(cut, good, W, H), W, H) != 0).any(), "the plain view enters below the root"
    centre = 0.5 * (root[0::2] + root[1::2])
    inside = good.copy()
    inside[:3] = centre                                              # the eye inside the root box
    # a cut box with a corner behind the eye: the eye beside cut box 0, level with its middle, looking along it
    b = cut.box[0]
    beside = good.copy()
    beside[:3] = [b[1] + 0.05 * (b[1] - b[0]), 0.5 * (b[2] + b[3]), 0.5 * (b[4] + b[5])]
    cases = {"inside": inside, "beside": beside}
    for k, v in ((3, np.nan), (0, np.inf), (7, -np.inf), (11, np.nan)):
        bad = good.copy()
        bad[k] = v
        cases[f"nonfinite{k}"] = bad
    for name, b12 in cases.items():
        rects = pkg.entry_rects(cut, b12, W, H)
        assert (rects == [0, 0xffff, 0, 0xffff]).all(), name
        assert (pkg.entry_tiles(cut, rects, W, H) == 0).all(), name
