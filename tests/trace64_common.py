"""Shared pieces of the double-precision ray-query tests (test_trace_cpu_f64.py, test_gpu_trace_f64.py):
the render<double> fixtures (tests/golden/f64/) with their rays rebuilt on the host, a numpy
Moller-Trumbore in float64, an exact fma for the reference CMake build's rays, the caller-style ray
sets, a brute-force answer that knows no BVH, and the checks both the CPU path and the GPU path must
pass (each takes a `trace(rays, mode, closest, occluded)` callable).

The double queries are pinned five ways: (1) the reference's own double records of the contraction-free
build through camera_rays64 / shadow_rays64, (2) its CMake build's records through rays rebuilt with a
correctly rounded fma, (3) brute force over all triangles, (4) GPU against CPU byte for byte, (5) the
reference's own traverse(ray, intersector) on stored caller rays (tests/golden/rays64/), ray by ray."""
import functools
import json
import os
from fractions import Fraction

import numpy as np

from conftest import GOLDEN, import_package

F64_DIR = os.path.join(GOLDEN, "f64")
D = np.float64
DBL_MAX = D(np.finfo(np.float64).max)

# (1) the exact build's records: tri1 (the root is a leaf), quad (one step, no stack), ...
EXACT_FIXTURES = ["tri1", "quad", "degenerate", "proc_101", "bunny_97x61_primary", "dragon_333x217"]
# ... the shadow flags of those rendered in full mode
OCCLUSION_FIXTURES = ["tri1", "quad", "degenerate", "proc_101", "dragon_333x217"]
# (2) the reference CMake build's records (64 x 48 each: the fma helper is exact, not fast)
REF_FIXTURES = ["tri1", "quad", "degenerate"]
DRAGON = "dragon_333x217"
TINY_FIXTURES = ["tri1", "quad"]
WINDOW_TMIN = np.asarray([0, -2, -np.inf, 1e-3], D)
WINDOW_TMAX = np.asarray([DBL_MAX, np.inf, 1, 0], D)


def _hex64(hx):
    return np.asarray([int(h, 16) for h in hx], np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def fixture(name, build="exact"):
    """(cfg, mesh, bvh, basis12, sun, meta, records) of a render<double> fixture: build "exact" -- the
    contraction-free reference build and a scene prepared with ARITH_EXACT; "ref" -- the reference's own
    CMake build (FMA contraction), ARITH_FMA.  basis / sun: the fixture's pinned bits."""
    pkg = import_package()
    cfg = pkg.configs.CONFIGS[name]
    with open(os.path.join(F64_DIR, name + ".json")) as f:
        meta = json.load(f)
    rec = dict(np.load(os.path.join(F64_DIR, name + (".ref" if build == "ref" else "") + ".records.npz")))
    for a in rec.values():
        a.setflags(write=False)
    mesh, bvh, _ = pkg.prepare(cfg, f64=True, arith=1 if build == "ref" else 0)
    bb, pose = (meta["ref_basis"], meta["ref_pose"]) if build == "ref" else (meta["basis"], meta["pose"])
    basis = np.concatenate([_hex64(pose["eye"]), _hex64(bb["dir"] + bb["u"] + bb["v"])])
    return cfg, mesh, bvh, basis, _hex64(pose["sun"]), meta, rec


def root_box(bvh):
    return np.ascontiguousarray(bvh.nodes[0, :6]).view(np.float64).copy()   # xmin, xmax, ymin, ymax, zmin, zmax


def dot(a, b):
    s = a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    return s + a[..., 2] * b[..., 2]


def moller_trumbore(tri, rays):
    """triangle.hpp:95-115 in float64 numpy, contraction-free: (t, u, v) of rays [n, 8] on triangles
    [n, 12] or, broadcast, [1, m, 12] against rays [n, 1, 8]."""
    p0, e1, e2, n = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9], tri[..., 9:12]
    o, d = rays[..., 0:3], rays[..., 3:6]
    with np.errstate(all="ignore"):
        c = p0 - o
        r = np.stack([d[..., 1] * c[..., 2] - d[..., 2] * c[..., 1], d[..., 2] * c[..., 0] - d[..., 0] * c[..., 2],
                      d[..., 0] * c[..., 1] - d[..., 1] * c[..., 0]], axis=-1)
        inv_det = D(1) / dot(n, d)
        return dot(n, c) * inv_det, dot(r, e2) * inv_det, dot(r, e1) * inv_det


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, D).view(np.uint64), np.ascontiguousarray(b, D).view(np.uint64))


def hits_equal(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_misses_are_zero(hits):
    """A miss is {-1, 0, 0.0, 0.0, 0.0}: all-zero bits after prim; the reserved word is 0 in every record."""
    miss = hits["prim"] < 0
    assert (hits["prim"][miss] == -1).all() and not hits["pad"].any()
    for k in ("t", "u", "v"):
        assert not hits[k][miss].view(np.uint64).any(), k


def fma(a, b, c):
    """fma(a, b, c) of three finite doubles, correctly rounded: the exact rational a b + c, rounded once."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def camera_rays64_fma(basis12, W, H):
    """The primary rays of ceres_render64<.., true> (the reference CMake build's contraction):
    a = dir + fma(iv, v, iu u), inv = 1 / sqrt(fma(az, az, fma(ax, ax, ay ay))), d = a inv."""
    b = np.asarray(basis12, D).reshape(12)
    eye, dir_, iu, iv = b[0:3], b[3:6], b[6:9], b[9:12]
    u = D(2) * (np.arange(W, dtype=D) + D(0.5)) / D(W) - D(1)
    v = D(2) * (np.arange(H, dtype=D) + D(0.5)) / D(H) - D(1)
    rays = np.empty((W * H, 8), D)
    rays[:, 0:3] = eye
    rays[:, 6] = 0
    rays[:, 7] = DBL_MAX
    for j in range(H):
        for i in range(W):
            a = np.asarray([dir_[k] + D(fma(iv[k], v[j], iu[k] * u[i])) for k in range(3)], D)
            s = D(fma(a[2], a[2], fma(a[0], a[0], a[1] * a[1])))
            rays[j * W + i, 3:6] = a * (D(1) / np.sqrt(s))
    return rays


def expected_hits(pkg, rec, n):
    """A fixture's records as hit32 records of its n = W*H camera rays (unrecorded pixels: none here)."""
    assert len(rec["pixel"]) == n
    exp = np.zeros(n, pkg.HIT64_DTYPE)
    exp["prim"] = -1
    hit = rec["prim"] >= 0
    px = rec["pixel"][hit]
    for k in ("prim", "t", "u", "v"):
        exp[k][px] = rec[k][hit]
    exp["prim"][rec["pixel"][~hit]] = -1
    return exp


# ---------------------------------------------------------------- (1), (2): the reference's records

def check_closest_against_fixture(pkg, trace, name, build="exact", check_stats=True):
    """Every pixel of the fixture: prim equal, t, u, v bit for bit, misses all-zero; the counters are
    the reference's Statistics of the primary rays."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(name, build)
    W, H = cfg["W"], cfg["H"]
    rays = pkg.camera_rays64(basis, W, H) if build == "exact" else camera_rays64_fma(basis, W, H)
    hits, _, st = trace(rays, pkg.MODE_FMA if build == "ref" else 0, True, False)
    exp = expected_hits(pkg, rec, W * H)
    assert hits.dtype == pkg.HIT64_DTYPE and hits.dtype.itemsize == 32
    assert np.array_equal(hits["prim"], exp["prim"]), name
    for k in ("t", "u", "v"):
        assert same_bits(hits[k], exp[k]), (name, k)
    assert_misses_are_zero(hits)
    assert hits_equal(hits, exp), name
    assert st["rays"] == W * H and st["hits"] == int((exp["prim"] >= 0).sum()) > 0
    if check_stats:
        assert st["node_pairs"] == meta[build]["primary_pairs"], name
        assert st["tri_tests"] == meta[build]["primary_tests"], name
    return rays, hits


def check_occlusion_against_fixture(pkg, trace, name):
    """The rebuilt shadow ray of every recorded hit: occluded == (shadow == 1), and the closest query
    of the same rays agrees ray by ray."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(name)
    hit = rec["prim"] >= 0
    hits = np.zeros(int(hit.sum()), pkg.HIT64_DTYPE)
    for k in ("prim", "t", "u", "v"):
        hits[k] = rec[k][hit]
    srays, idx = pkg.shadow_rays64(mesh, hits, sun)
    assert len(idx) == len(hits) > 0 and srays.dtype == D
    _, occ, st = trace(srays, 0, False, True)
    assert np.array_equal(occ, (rec["shadow"][hit] == 1).astype(np.uint8)), name
    assert st["rays"] == len(srays) and st["hits"] == int(occ.sum())
    h2, occ2, _ = trace(srays, 0, True, True)
    assert np.array_equal(occ2, occ) and np.array_equal(h2["prim"] >= 0, occ == 1)
    assert_misses_are_zero(h2)


# ---------------------------------------------------------------- (3): brute force, independent of any walk

BRUTE_SCENES = ["proc33", "quad"]
BRUTE_N = 1637
BRUTE_SEED = {"proc33": 20261101, "quad": 20261102}
BRUTE_TIE_SHARE = 0.01                                                # at most 1 % of the rays may be excluded
# Non-tied rays that the reference's walk answers differently from the brute force because its slab
# test culls the hit, worked by hand from node_intersectors.hpp: {scene: {ray index: reason}}.  They
# count inside the same 1 %.
BRUTE_CULLED = {"proc33": {}, "quad": {}}


@functools.lru_cache(maxsize=None)
def brute_scene(which):
    """(mesh, bvh): proc_mesh_f64(33), the 32 x 32 heightfield of 2,048 triangles, or the quad fixture."""
    pkg = import_package()
    if which == "proc33":
        mesh = pkg.proc_mesh_f64(33)
        assert len(mesh) == 2048
        return mesh, pkg.build_bvh(mesh)
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["quad"], f64=True)
    return mesh, bvh


@functools.lru_cache(maxsize=None)
def brute_rays(which):
    """1,637 caller-style rays in float64, fixed seed: origins up to 2.5 half-extents from the root
    box's centre (around and inside the box), half of them aimed at a triangle's centroid, the others
    at a point of the box; direction (target - origin) 2^k, k in [-20, 20], reversed for one ray in
    four; one ray in eight has a component exactly +0 or -0 (its origin moved so it still passes its
    target); windows from {0, -2, -inf, 1e-3} x {DBL_MAX, +inf, 1, 0}; the last eight rays are aimed to
    hit under tmin > tmax (twice), tmin = +inf, tmax = -inf and a NaN as tmin, as tmax and as both (twice)."""
    mesh, bvh = brute_scene(which)
    b = root_box(bvh)
    c, h = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2
    h = np.maximum(h, h.max() / 2)                                    # a flat box still gets origins off its plane
    rng = np.random.default_rng(BRUTE_SEED[which])
    n = BRUTE_N
    aimed = rng.integers(0, 2, n) == 1
    aimed[-8:] = True
    tr = mesh.tri[rng.integers(0, len(mesh), n)]
    centroid = tr[:, 0:3] + (tr[:, 6:9] - tr[:, 3:6]) / 3             # p0, p0 - e1, p0 + e2
    target = np.where(aimed[:, None], centroid, c + h * rng.uniform(-1, 1, (n, 3)))
    origin = c + 2.5 * h * rng.uniform(-1, 1, (n, 3))
    scale = np.exp2(rng.integers(-20, 21, n)) * np.where(rng.integers(0, 4, n) == 0, -1.0, 1.0)
    scale[-8:] = 1.0
    zero = np.zeros(n, bool)
    zero[0:n - 8:8] = True
    axis = rng.integers(0, 3, n)
    origin[zero, axis[zero]] = target[zero, axis[zero]]
    d = (target - origin) * scale[:, None]
    d[zero, axis[zero]] = np.where(rng.integers(0, 2, int(zero.sum())) == 1, -0.0, 0.0)
    rays = np.zeros((n, 8), D)
    rays[:, 0:3] = origin
    rays[:, 3:6] = d
    rays[:, 6] = WINDOW_TMIN[rng.integers(0, 4, n)]
    rays[:, 7] = WINDOW_TMAX[rng.integers(0, 4, n)]
    nan = np.nan
    rays[-8:, 6:8] = np.asarray([[2, 1], [1e-3, 0], [np.inf, DBL_MAX], [0, -np.inf], [nan, DBL_MAX], [0, nan], [nan, nan],
                                 [nan, 1]], D)
    assert (rays[:, 3:6] != 0).any(axis=1).all()
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def brute_expected(which):
    """The answer in contraction-free numpy float64, from every (ray, triangle) pair: the minimum t
    over the triangles with u, v, w >= 0 and t inside the ray's window.  Returns {prim, t, u, v of the
    winner (prim -1: a miss), tied: the minimum is attained by two triangles (the winner would depend
    on the visit order: such rays are excluded), open_hit: a hit under the window [-inf, +inf]}."""
    mesh, _ = brute_scene(which)
    rays = brute_rays(which)
    n = len(rays)
    prim = np.full(n, -1, np.int64)
    best = np.zeros((n, 3), D)
    tied = np.zeros(n, bool)
    open_hit = np.zeros(n, bool)
    tri = mesh.tri[None, :, :]
    for k0 in range(0, n, 256):
        r = rays[k0:k0 + 256]
        t, u, v = moller_trumbore(tri, r[:, None, :])
        with np.errstate(invalid="ignore"):
            inside = (u >= 0) & (v >= 0) & (D(1) - u - v >= 0)
            ok = inside & (t >= r[:, 6:7]) & (t <= r[:, 7:8])
            open_hit[k0:k0 + 256] = (inside & (t >= -np.inf) & (t <= np.inf)).any(axis=1)
        tt = np.where(ok, t, np.inf)
        win = tt.argmin(axis=1)
        rows = np.arange(len(r))
        has = ok.any(axis=1)
        tmin = tt[rows, win]
        tied[k0:k0 + 256] = has & ((ok & (t == tmin[:, None])).sum(axis=1) > 1)
        prim[k0:k0 + 256] = np.where(has, win, -1)
        for j, a in enumerate((t, u, v)):
            best[k0:k0 + 256, j] = np.where(has, a[rows, win], 0.0)
    return {"prim": prim, "t": best[:, 0], "u": best[:, 1], "v": best[:, 2], "tied": tied, "open_hit": open_hit}


def check_brute_conditions(which):
    """What the brute-force comparison needs, from numpy alone (no code under test runs here): at most
    1 % of the rays excluded (ties and hand-worked culls together), at least 10 % hits and 10 % misses
    among the others, and a hit that the ray's own window rejects."""
    rays, exp = brute_rays(which), brute_expected(which)
    n = len(rays)
    assert n == BRUTE_N
    culled = np.zeros(n, bool)
    culled[list(BRUTE_CULLED[which])] = True
    excluded = exp["tied"] | culled
    assert excluded.sum() <= BRUTE_TIE_SHARE * n, (which, int(excluded.sum()))
    keep = ~excluded
    hit = exp["prim"] >= 0
    assert (hit & keep).sum() >= 0.10 * n and (~hit & keep).sum() >= 0.10 * n, (which, int(hit.sum()))
    assert (exp["open_hit"] & ~hit & keep).any(), which              # the ray's own window rejects a hit
    special = np.arange(n - 8, n)
    assert exp["open_hit"][special].all() and not hit[special].any(), which
    assert ((rays[:, 3:6] == 0).any(axis=1) & hit).any(), which       # a ray with a zero component hits
    return keep


def check_against_brute_force(pkg, trace, which):
    """Every non-excluded ray: the brute-force winner, and (t, u, v) bitwise the numpy values of the
    reported triangle; occlusion == "some triangle is accepted"."""
    keep = check_brute_conditions(which)
    mesh, _ = brute_scene(which)
    rays, exp = brute_rays(which), brute_expected(which)
    hits, occ, st = trace(np.array(rays), 0, True, True)
    assert_misses_are_zero(hits)
    bad = np.flatnonzero(keep & (hits["prim"] != exp["prim"]))
    assert len(bad) == 0, (which, "rays that disagree with the brute force", bad[:16].tolist())
    assert np.array_equal(occ[keep], (exp["prim"][keep] >= 0).astype(np.uint8)), which
    got = hits["prim"] >= 0                                           # tied rays too: the reported triangle's own values
    t, u, v = moller_trumbore(mesh.tri[hits["prim"][got]], rays[got])
    assert same_bits(hits["t"][got], t) and same_bits(hits["u"][got], u) and same_bits(hits["v"][got], v), which
    for k in ("t", "u", "v"):
        assert same_bits(hits[k][keep], exp[k][keep]), (which, k)
    assert st["rays"] == len(rays) and st["hits"] == int(got.sum())


# ---------------------------------------------------------------- (4): the sets of GPU against CPU

@functools.lru_cache(maxsize=None)
def adversarial_rays():
    """trace_common.adversarial_rays()'s recipe in float64 against the double dragon_333x217 scene:
    4,099 rays, fixed seed -- origins uniform in twice the root box, random unnormalised directions
    scaled by 2^k (k in [-20, 20]), one ray in eight with a component exactly +0 or -0, windows from
    tmin {0, -2, -inf, 1e-3} x tmax {DBL_MAX, +inf, 1, 0}; then the six axis directions from inside and
    from outside the box, a zero direction, NaN / +-inf in an origin and in a direction, tmin > tmax."""
    _, _, bvh, _, _, _, _ = fixture(DRAGON)
    b = root_box(bvh)
    lo, hi = b[0::2], b[1::2]
    c, h = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(20261019)
    n = 4099
    rays = np.zeros((n, 8), D)
    rays[:, 0:3] = c + 2 * h * rng.uniform(-1, 1, (n, 3))
    rays[:, 3:6] = rng.normal(size=(n, 3)) * np.exp2(rng.integers(-20, 21, n))[:, None]
    eighth = np.arange(0, n, 8)
    rays[eighth, 3 + rng.integers(0, 3, len(eighth))] = np.where(rng.integers(0, 2, len(eighth)) == 1, -0.0, 0.0)
    rays[:, 6] = WINDOW_TMIN[rng.integers(0, 4, n)]
    rays[:, 7] = WINDOW_TMAX[rng.integers(0, 4, n)]
    k = n - 21
    special = []
    inside = c + 0.25 * h * rng.uniform(-1, 1, 3)
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = np.zeros(3, D)
            e[axis] = sign
            outside = inside.copy()
            outside[axis] = c[axis] - sign * 3 * h[axis]              # in front of the box, looking at it
            special.append(np.concatenate([inside, e, [0, DBL_MAX]]))
            special.append(np.concatenate([outside, e, [0, DBL_MAX]]))
    one = np.asarray([0.3, -1.0, 0.2], D)
    special.append(np.concatenate([inside, [0, 0, 0], [0, DBL_MAX]]))
    for bad in (np.nan, np.inf, -np.inf):
        o = inside.copy()
        o[1] = bad
        special.append(np.concatenate([o, one, [0, DBL_MAX]]))
        dd = one.copy()
        dd[2] = bad
        special.append(np.concatenate([inside, dd, [0, DBL_MAX]]))
    special.append(np.concatenate([inside, one, [2, 1]]))             # tmin > tmax
    special.append(np.concatenate([inside, one, [np.inf, -np.inf]]))
    assert len(special) == 21
    rays[k:] = np.asarray(special, D)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def tiny_tree_rays(name):
    """trace_common.tiny_tree_rays' recipe in float64: 357 rays (five wavefronts and a tail of 37)
    against tri1 (the root is a leaf) or quad (a root with two leaf children), each aimed from around
    the scene at a point of a triangle's plane, inside the triangle or past its edges, scaled by 2^k
    (k in [-4, 4]) and reversed for one ray in four; the adversarial windows, the last four rays with
    tmin > tmax."""
    _, mesh, bvh, _, _, _, _ = fixture(name)
    assert (bvh.nodes[0, 6] != 0) == (name == "tri1")                 # primitive_count of the root: tri1's is a leaf
    b = root_box(bvh)
    c, h = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2
    h = np.maximum(h, h.max() / 2)
    rng = np.random.default_rng(20261020)
    n = 357
    tr = mesh.tri
    k = rng.integers(0, len(tr), n)
    target = tr[k, 0:3] + rng.uniform(-0.6, 1.2, (n, 1)) * tr[k, 3:6] + rng.uniform(-0.6, 1.2, (n, 1)) * tr[k, 6:9]
    rays = np.zeros((n, 8), D)
    rays[:, 0:3] = c + 3 * h * rng.uniform(-1, 1, (n, 3))
    scale = np.exp2(rng.integers(-4, 5, n)) * np.where(rng.integers(0, 4, n) == 0, -1.0, 1.0)
    rays[:, 3:6] = (target - rays[:, 0:3]) * scale[:, None]
    rays[:, 6] = WINDOW_TMIN[rng.integers(0, 4, n)]
    rays[:, 7] = WINDOW_TMAX[rng.integers(0, 4, n)]
    rays[-4:, 6:8] = np.asarray([[2, 1], [np.inf, -np.inf], [1e-3, 0], [1, -2]], D)
    rays.setflags(write=False)
    return rays


def check_tiny_tree_input(name, hits, hits_open):
    """What keeps the smallest-trees comparison from passing vacuously.  hits: the CPU path's closest
    hits of tiny_tree_rays(name); hits_open: of the same rays under [0, DBL_MAX]."""
    hit = hits["prim"] >= 0
    assert hit.any() and (~hit).any(), name
    assert ((hits_open["prim"] >= 0) & ~hit).any(), name             # the ray's own window rejects a hit


def check_adversarial_input(rays, hits):
    """The adversarial set does hit the mesh, does miss it, and holds the non-finite rays."""
    hit = hits["prim"] >= 0
    assert hit.sum() > 100 and (~hit).sum() > 100
    assert np.isnan(rays[:, 0:6]).any() and np.isinf(rays[:, 0:6]).any() and (rays[:, 3:6] == 0).all(axis=1).any()


def modes(pkg):
    """{exact, FMA}: (mode, fixture build)."""
    return [(0, "exact"), (pkg.MODE_FMA, "ref")]


# ---------------------------------------------------------------- rays the reference traced itself
# tests/golden/rays64/<set>.npz (tests/golden/make_golden_rays.py): caller-style ray64 records and what
# the reference's own traverser.traverse(ray, intersector, statistics) returned for each in its two
# double builds (the product's double path has no robust mode, so only the fast intersector is stored).

RAY_SETS64 = ["dragon_adversarial64", "tri1_tiny64", "quad_tiny64", "lattice_ties64"]
RAY_VARIANTS64 = ["exact_fast", "ref_fast"]
RAY_FIELDS = ("prim", "t", "u", "v", "occluded", "steps", "tests")
RAYS64_DIR = os.path.join(GOLDEN, "rays64")
_SET_FIXTURE = {"dragon_adversarial64": DRAGON, "tri1_tiny64": "tri1", "quad_tiny64": "quad"}
LATTICE64 = "lattice_ties64"


def variant_mode(pkg, variant):
    """(mode, fixture build) of a stored variant."""
    return dict(zip(RAY_VARIANTS64, modes(pkg)))[variant]


@functools.lru_cache(maxsize=None)
def lattice64(build="exact"):
    """(cfg, mesh, bvh) of tests/golden/lattice.obj as a double scene."""
    import trace_common as tc
    pkg = import_package()
    cfg = tc.lattice(0)[0]
    mesh, bvh, _ = pkg.prepare(cfg, f64=True, arith=1 if build == "ref" else 0)
    return cfg, mesh, bvh


def ray_set_rays(name):
    """The generator of a double set's rays (the fixture stores its output): the adversarial and the
    smallest-trees sets of this module, and trace_common's lattice rays widened to double."""
    if name == LATTICE64:
        import trace_common as tc
        return tc.lattice_rays().astype(D)
    if name == "dragon_adversarial64":
        return adversarial_rays()
    return tiny_tree_rays(_SET_FIXTURE[name])


def ray_set_config(name):
    """The config whose scene a double set's rays are traced against."""
    return lattice64()[0] if name == LATTICE64 else import_package().configs.CONFIGS[_SET_FIXTURE[name]]


def ray_set_scene(name, build="exact"):
    """(mesh, bvh) of a double set's scene in the given build's arithmetic."""
    return lattice64(build)[1:3] if name == LATTICE64 else fixture(_SET_FIXTURE[name], build)[1:3]


@functools.lru_cache(maxsize=None)
def load_ray_fixture64(name):
    """tests/golden/rays64/<name>.npz: {"rays": float64 [n, 8], variant: {prim, t, u, v (uint64 bits),
    occluded, steps, tests}}; read-only arrays, loaded once."""
    z = np.load(os.path.join(RAYS64_DIR, name + ".npz"))
    out = {"rays": z["rays"]}
    for v in RAY_VARIANTS64:
        out[v] = {k: z[v + "_" + k] for k in RAY_FIELDS}
    for a in [out["rays"]] + [a for v in RAY_VARIANTS64 for a in out[v].values()]:
        a.setflags(write=False)
    assert out["rays"].dtype == D and out["rays"].shape[1] == 8
    assert all(out[v][k].dtype == np.uint64 for v in RAY_VARIANTS64 for k in ("t", "u", "v"))
    return out


def reference_hits(pkg, ref):
    """A variant's records as the API's hit32 array {prim, pad, t, u, v}."""
    exp = np.zeros(len(ref["prim"]), pkg.HIT64_DTYPE)
    exp["prim"] = ref["prim"]
    for k in ("t", "u", "v"):
        exp[k] = ref[k].view(D)
    return exp


def check_against_ray_fixture64(pkg, trace, name, variant, stats, closest=True, occluded=True):
    """trace(rays, mode, closest, occluded) on the set's double scene prepared for `variant` must return
    the reference's own answer for every stored ray: prim equal, t, u, v bit for bit, misses all-zero
    after prim, occluded equal; counters rays = n and hits = the reference's hit count.  stats (the CPU
    path, GPU stats scenes): the rays none of whose eight doubles is NaN go in one call, the others in
    a call of their own, and each call's node_pairs / tri_tests are the sums of the reference's
    traversal_steps / intersections of the closest walk over its rays.  Otherwise one call in stored
    order."""
    fx = load_ray_fixture64(name)
    ref = fx[variant]
    mode, _ = variant_mode(pkg, variant)
    exp_h, exp_o = reference_hits(pkg, ref), ref["occluded"].astype(np.uint8)
    assert_misses_are_zero(exp_h)
    miss = exp_h["prim"] < 0
    idx = np.arange(len(fx["rays"]))
    parts = [idx]
    if stats:
        nan = np.isnan(fx["rays"]).any(axis=1)
        parts = [idx[~nan]] + ([idx[nan]] if nan.any() else [])
    for k, part in enumerate(parts):
        rays = np.ascontiguousarray(fx["rays"][part])
        hits, occ, st = trace(rays, mode, closest, occluded)
        where = (name, variant, "stats" if stats else "production", "part %d" % k)
        if closest:
            assert hits.dtype == pkg.HIT64_DTYPE, where
            assert np.array_equal(hits["prim"], exp_h["prim"][part]), (where, np.flatnonzero(hits["prim"] != exp_h["prim"][part])[:8])
            for f in ("t", "u", "v"):
                assert same_bits(hits[f], exp_h[f][part]), (where, f)
            assert_misses_are_zero(hits)
            assert hits.tobytes() == exp_h[part].tobytes(), where
        if occluded:
            assert np.array_equal(occ, exp_o[part]), (where, np.flatnonzero(occ != exp_o[part])[:8])
        assert st["rays"] == len(part), where
        assert st["hits"] == int((~miss[part]).sum() if closest else exp_o[part].sum()), where
        if stats and closest:
            assert st["node_pairs"] == int(ref["steps"][part].sum(dtype=np.uint64)), where
            assert st["tri_tests"] == int(ref["tests"][part].sum(dtype=np.uint64)), where
