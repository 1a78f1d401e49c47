"""Shared by tests/test_soups_cpu.py, tests/test_gpu_soups.py and tests/golden/make_golden_soups.py:
deterministic triangle soups with non-finite, huge and denormal coordinates -- what a simulation that
blew up hands to the builders and the scene upkeep calls -- as bvh::Triangle<float> rows
{p0, e1 = p0 - p1, e2 = p2 - p0, n}.

The base of every soup is the finite "uniform" soup of test_gpu_bvh.py (three vertices uniform in
[-5, 5)^3), a function of n alone.  A kind poisons max(1, n // 16) of its rows (at most 6.25 % for
n >= 16; at n = 1 and 2 one row is the least there is), so the finite part still makes a scene one can
render; `all_nan` and `denormal` change every row.  What the reference does with such rows
(bounding_box.hpp:23-27 is std::min / std::max, triangle.hpp:39-48 seeds the box with p0):

  nan_p0     one component of p0 is +NaN, -NaN or a NaN with a payload: the box seeded from it keeps the
             NaN, the sequential root fold and every bin fold drop it (a NaN that arrives second loses),
             the NaN centre goes to bin 0.  nan_p0_first / nan_p0_last also poison row 0 / row n - 1.
  nan_edge   p0 finite, a NaN in e1 or e2: p1 / p2 are NaN and the per-primitive extend drops them; the
             centre is NaN.
  inf        +-inf in p0; every other row of the share has p0 = e1 = +-inf in one component, so p0 - e1
             is inf - inf: the default NaN, negative on x86 and positive on the GPU, which no node may show.
  huge       finite vertices of magnitude (2.7e38, 3e38], one sign per axis within a triangle and other signs
             in other triangles: every vertex, edge and primitive box is finite, but hi - lo of a node
             overflows, center_to_bin is 0 with a finite offset, half areas and SAH costs are inf or NaN,
             `cost < best` is never true and the build falls to the 0.4-quantile split or the n <= 16 leaf rule.
  denormal   every coordinate in [1e-45, 1e-39]: 1 / diag overflows, center_to_bin is inf.
  all_nan    every component of every p0 is a NaN: the root stays the empty box +-FLT_MAX.
  mixed      the poisoned share dealt round-robin over nan_p0, nan_edge, inf, inf - inf, huge and
             denormal rows.
  mixed_nan  the same without the inf, inf - inf and huge rows.  One infinite or huge row makes the root's
             diagonal infinite, center_to_bin 0 and every split one-sided: the reference's tree of `inf`,
             `huge` and `mixed` above 16 triangles is ONE leaf (as is `denormal`'s, through an infinite
             center_to_bin).  This kind keeps a finite root and a real tree under it.
"""
import hashlib

import numpy as np

SEED = 20261                                     # chosen on the CPU path, see test_soups_cpu.py's guards
SIZES = (1, 2, 17, 200, 300, 2049, 4097, 9000)   # leaf root; k_small; just over the small-subtree
                                                 # threshold (256); k_init's 2048 / block + 1; k_bin's 4096
                                                 # chunk + 1; several large levels
SOME = (200, 300, 4097)
KINDS = ("nan_p0", "nan_p0_first", "nan_p0_last", "nan_edge", "inf", "huge", "denormal", "all_nan", "mixed", "mixed_nan")
EVERY_SIZE = ("mixed", "nan_p0", "mixed_nan")
CASES = ([(k, n) for k in EVERY_SIZE for n in SIZES] +
         [(k, n) for k in KINDS if k not in EVERY_SIZE for n in SOME])
IDS = ["%s-%d" % c for c in CASES]
RENDERED = (("mixed", 4097), ("nan_p0", 300), ("mixed_nan", 4097), ("huge", 4097))    # the soups the scene tests render
FRAMES = (("mixed", 4097), ("mixed_nan", 4097))  # the soups whose reference frame the fixture records
FRAME_W, FRAME_H = 97, 61

NANS = (0x7fc00000, 0xffc00000, 0x7f800001, 0xffabcdef)
FLT_MAX = np.float32(3.4028234663852886e38)


def _rows(p):
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        e1 = p0 - p1
        e2 = p2 - p0
        nrm = np.cross(e1, e2).astype(np.float32)
    return np.concatenate([p0, e1, e2, nrm], axis=1).astype(np.float32)


def base(n, seed=SEED):
    """The finite uniform soup of n triangles."""
    rng = np.random.default_rng([seed, n])
    return _rows(rng.random((n, 3, 3), dtype=np.float32) * 10 - 5)


def share(n):
    return max(1, n // 16)


def _nan(k):
    return np.array([NANS[k % 4]], np.uint32).view(np.float32)[0]


def _poison(tri, u, row, what, k, rng):
    """Poison one row in place; k numbers the poisoned rows (it deals the patterns)."""
    c = int(rng.integers(0, 3))
    if what == "nan_p0":
        u[row, c] = NANS[k % 4]
    elif what == "nan_edge":
        u[row, 3 + 3 * (k % 2) + c] = NANS[(k // 2) % 4]
    elif what == "inf":
        tri[row, c] = np.float32(np.inf if k % 2 else -np.inf)
    elif what == "infinf":
        tri[row, c] = tri[row, 3 + c] = np.float32(np.inf if k % 2 else -np.inf)
    elif what == "huge":
        # one sign per axis within the triangle (it varies across triangles), magnitudes in (2.7e38, 3e38]:
        # the three vertices and both edges stay finite, only differences ACROSS triangles overflow
        sign = np.where(rng.random((1, 1, 3)) < 0.5, np.float32(-1), np.float32(1)).astype(np.float32)
        mag = (np.float32(3e38) * (np.float32(1) - np.float32(0.1) * rng.random((1, 3, 3), dtype=np.float32))).astype(np.float32)
        mag[0, 0, :] = np.float32(3e38)                                # p0 is exactly +-3e38
        tri[row] = _rows(sign * mag)[0]
    elif what == "denormal":
        tri[row] = _rows(_denormal(rng, 1))[0]
    elif what == "all_nan":
        for a in range(3):
            u[row, a] = NANS[(k + a) % 4]
    else:
        raise ValueError(what)


def _denormal(rng, n):
    bits = rng.integers(1, 713549, size=(n, 3, 3)).astype(np.uint32)      # 1 = 1.4e-45 ... 713548 < 1e-39
    return bits.view(np.float32)


MIXED = ("nan_p0", "nan_edge", "inf", "infinf", "huge", "denormal")
MIXED_NAN = ("nan_p0", "nan_edge", "denormal")


def soup(kind, n, seed=SEED):
    """(tri [n, 12] float32, poisoned [n] bool) of a kind; the rest of tri equals base(n, seed)."""
    tri = base(n, seed)
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    marked = np.zeros(n, bool)
    if kind == "denormal":
        return _rows(_denormal(rng, n)), ~marked
    rows = np.arange(n) if kind == "all_nan" else np.sort(rng.choice(n, share(n), replace=False))
    if kind == "nan_p0_first":
        rows[0] = 0
    if kind == "nan_p0_last":
        rows[-1] = n - 1
    u = tri.view(np.uint32)
    for k, row in enumerate(rows):
        what, j = kind, k                                             # j deals the patterns of one sort of row
        if kind in ("nan_p0_first", "nan_p0_last"):
            what = "nan_p0"
        elif kind == "inf":
            what, j = ("infinf" if k % 2 else "inf"), k // 2
        elif kind in ("mixed", "mixed_nan"):
            deal = MIXED if kind == "mixed" else MIXED_NAN
            what, j = deal[k % len(deal)], k // len(deal)
        _poison(tri, u, int(row), what, j, rng)
    marked[rows] = True
    return tri, marked


def nonfinite_rows(tri):
    """Rows with a non-finite input value in p0, e1 or e2."""
    return ~np.isfinite(tri[:, :9]).all(axis=1)


def finite_box(tri):
    """{x0, x1, y0, y1, z0, z1} of the vertices of the rows whose vertices are all finite and below 1e30."""
    with np.errstate(all="ignore"):
        t = tri.astype(np.float64)
        v = np.stack([t[:, 0:3], t[:, 0:3] - t[:, 3:6], t[:, 0:3] + t[:, 6:9]], axis=1)
        ok = (np.isfinite(v) & (np.abs(v) < 1e30)).all(axis=(1, 2))
    v = v[ok].reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2])]


def frame_camera(box):
    """(eye, dir, up, fov) of tile_compact_model.look(root = box): two diagonals in front of the centre."""
    lo, hi = np.array(box[0::2]), np.array(box[1::2])
    eye = (lo + hi) / 2 + np.array([0.0, 0.0, -2.0 * float(np.linalg.norm(hi - lo))])
    return eye.astype(np.float32), np.array([0, 0, 1], np.float32), np.array([0, 1, 0], np.float32), 40.0


def sun_of(box):
    """A sun four diagonals from the finite part's centre (as test_gpu_cull._cameras places it)."""
    lo, hi = np.array(box[0::2]), np.array(box[1::2])
    return ((lo + hi) / 2 + np.array([-2.0, 3.0, -1.5]) / np.sqrt(15.25) * 4 * np.linalg.norm(hi - lo)).astype(np.float32)


def normals(tri):
    """Per-vertex normals of a soup: the unit face normal three times; zero where it is not finite."""
    n = tri[:, 9:12].astype(np.float64)
    with np.errstate(all="ignore"):
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        u = np.where(np.isfinite(ln) & (ln > 0), n / ln, 0.0)
    u = np.where(np.isfinite(u).all(axis=1, keepdims=True), u, 0.0)
    return np.tile(u, (1, 3)).astype(np.float32)


def sha(tri):
    return hashlib.sha256(np.ascontiguousarray(tri, np.float32).tobytes()).hexdigest()


# ---- what the scene tests share (pkg: the imported package)
def mesh_of(pkg, kind, n):
    tri, _ = soup(kind, n)
    return pkg.Mesh(tri, normals(tri))


def base_mesh(pkg, n):
    tri = base(n)
    return pkg.Mesh(tri, normals(tri))


def views(pkg, box, W, H):
    """The `centre`, `side` and `far` views of test_gpu_entry_nodes._views on the finite part's box."""
    import tile_compact_model as C
    return np.stack([C.look(pkg, box, W, H), C.look(pkg, box, W, H, yaw=9.0, pitch=-4.0, dist=2.5), C.look(pkg, box, W, H, dist=4.0)])


def root_of(bvh):
    return [float(x) for x in bvh.nodes[0, :6].view(np.float32)]


def batch_guard(pkg, mesh, bvh, b12, W, H):
    """On the host: the frames' cull rectangles under the BVH's root box, the tiles they cull, the scene's
    cut and the tiles that enter below the root (ceres_entry_rects / ceres_entry_tiles)."""
    import cull_fill_model as M
    import tile_compact_model as C
    root = root_of(bvh)
    with np.errstate(all="ignore"):
        rects = [M.cull_rect(b, root, W, H) for b in b12]
    out = dict(rects=rects, keep=[r == M.KEEP for r in rects], culled=0, below=0, cut=None)
    if bvh.nodes[0, 6]:                                               # a root leaf: no cut, no cull
        return out
    culled = C.culled_tiles(rects, W, H)
    out["culled"] = int(culled.sum())
    pairs, _, rlc = pkg.entry_relayout(mesh, bvh)
    cut = pkg.entry_cut(pairs, rlc, root)
    out["cut"] = cut
    if cut.entry_ok:
        for f, b in enumerate(b12):
            ent = pkg.entry_tiles(cut, pkg.entry_rects(cut, b, W, H), W, H)
            out["below"] += int(((ent != 0) & (ent != pkg.ENTRY_EMPTY) & ~culled[f]).sum())
    return out
