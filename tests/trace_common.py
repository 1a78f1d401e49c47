"""Shared pieces of the ray-query tests (test_trace_cpu.py, test_gpu_trace.py): the fixtures' scenes
and rebuilt rays, a numpy Moller-Trumbore, the caller-style ray sets with the loader of the reference's
answers to them (tests/golden/rays/), and the checks that both the CPU path and the GPU path must
pass (each takes a `trace(rays, mode, closest, occluded)` callable)."""
import functools
import os

import numpy as np

from conftest import GOLDEN, import_package, load_golden

# the fixtures whose records pin the closest query (tests/golden/<name>.records.npz: the
# contraction-free reference build's per-pixel {prim, t, u, v, shadow})
CLOSEST_FIXTURES = ["tri1", "quad", "dupleaf", "degenerate", "bunny_1x1", "bunny_97x61_primary", "dragon_333x217", "proc_101",
                    "quad_65x49_robust", "degenerate_65x49_robust", "bunny_97x61_primary_robust"]
OCCLUSION_FIXTURES = ["dupleaf", "bunny_1x1", "dragon_333x217", "proc_101", "tri1", "quad"]
DRAGON = "dragon_333x217"
F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)


def _bits(hexes):
    return np.asarray([int(h, 16) for h in hexes], np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name, arith=0):
    """(cfg, mesh, bvh, basis12, sun, meta, records) of a golden config; exact arithmetic: the pinned
    basis bits of the fixture (as smoke() does), otherwise the camera's own basis."""
    pkg = import_package()
    cfg = pkg.configs.CONFIGS[name]
    meta, rec, _ = load_golden(name)
    mesh, bvh, cam = pkg.prepare(cfg, arith=arith)
    if arith == 0:
        bb = meta["basis"]
        basis = np.concatenate([_bits(meta["pose"]["eye"]), _bits(bb["dir"]), _bits(bb["u"]), _bits(bb["v"])]).astype(F)
        sun = _bits(meta["pose"]["sun"])
    else:
        basis = cam.basis(cfg["W"], cfg["H"])
        sun = pkg.pose(cfg, arith=arith)[1]
    return cfg, mesh, bvh, basis, sun, meta, rec


def mode_of(pkg, name):
    return pkg.MODE_ROBUST if pkg.configs.CONFIGS[name].get("robust") else 0


def root_box(bvh):
    return bvh.nodes[0, :6].copy().view(np.float32)                   # xmin, xmax, ymin, ymax, zmin, zmax


def dot(a, b):
    s = a[:, 0] * b[:, 0]
    s = s + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def moller_trumbore(mesh, rays, prim):
    """triangle.hpp:95-115 in float32 numpy, contraction-free: (t, u, v) of ray k on triangle prim[k]."""
    tr = mesh.tri[prim]
    p0, e1, e2, n = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9], tr[:, 9:12]
    o, d = rays[:, 0:3], rays[:, 3:6]
    c = p0 - o
    r = np.stack([d[:, 1] * c[:, 2] - d[:, 2] * c[:, 1], d[:, 2] * c[:, 0] - d[:, 0] * c[:, 2],
                  d[:, 0] * c[:, 1] - d[:, 1] * c[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        inv_det = F(1) / dot(n, d)
        return dot(n, c) * inv_det, dot(r, e2) * inv_det, dot(r, e1) * inv_det


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def hits_equal(a, b):
    return a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the checks

def check_closest_against_fixture(pkg, trace, name, check_stats=True):
    """Every recorded pixel of the fixture: prim, t, u, v bit for bit, misses {-1, 0, 0, 0}; the
    traversal counters equal the reference's Statistics of the primary rays (the visiting order)."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(name)
    W, H = cfg["W"], cfg["H"]
    rays = pkg.camera_rays(basis, W, H)
    hits, _, st = trace(rays, mode_of(pkg, name), True, False)
    px = rec["pixel"]
    got = hits[px]
    assert np.array_equal(got["prim"], rec["prim"]), name
    miss = rec["prim"] < 0
    for k in ("t", "u", "v"):
        assert same_bits(got[k][~miss], rec[k][~miss]), (name, k)
        assert not got[k][miss].view(np.uint32).any(), (name, k)
    all_miss = hits["prim"] < 0
    assert not hits["t"][all_miss].view(np.uint32).any() and not hits["u"][all_miss].view(np.uint32).any()
    assert not hits["v"][all_miss].view(np.uint32).any()
    assert st["rays"] == W * H and st["hits"] == int(np.count_nonzero(~all_miss))
    if check_stats:
        assert st["node_pairs"] == meta["exact"]["primary_pairs"], name
        assert st["tri_tests"] == meta["exact"]["primary_tests"], name
    return rays, hits


def check_occlusion_against_fixture(pkg, trace, name):
    """The rebuilt shadow ray of every recorded hit pixel: occluded == (shadow == 1)."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(name)
    hit = rec["prim"] >= 0
    hits = np.zeros(int(hit.sum()), pkg.HIT_DTYPE)
    for k in ("prim", "t", "u", "v"):
        hits[k] = rec[k][hit]
    srays, idx = pkg.shadow_rays(mesh, hits, sun)
    assert len(idx) == len(hits)
    _, occ, st = trace(srays, mode_of(pkg, name), False, True)
    assert np.array_equal(occ, (rec["shadow"][hit] == 1).astype(np.uint8)), name
    assert st["hits"] == int(occ.sum())
    # ... and the closest query of the same rays agrees ray by ray
    h2, occ2, _ = trace(srays, mode_of(pkg, name), True, True)
    assert np.array_equal(occ2, occ) and np.array_equal(h2["prim"] >= 0, occ == 1)


def check_scale(pkg, trace):
    """A direction scaled by 2^k leaves prim, u, v alone and scales t by 2^-k, exactly."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(DRAGON)
    rays = pkg.camera_rays(basis, cfg["W"], cfg["H"])
    keep = (np.abs(rays[:, 3:6]) >= F(2.0 ** -20)).all(axis=1)
    assert keep.sum() > 50000
    exp = np.zeros(len(rays), pkg.HIT_DTYPE)
    exp["prim"] = -1
    for k in ("prim", "t", "u", "v"):
        exp[k][rec["pixel"]] = rec[k]
    exp = exp[keep]
    for scale, tscale in ((2.0, 0.5), (256.0, 2.0 ** -8)):
        r = rays[keep].copy()
        r[:, 3:6] *= F(scale)
        hits, _, _ = trace(r, 0, True, False)
        assert np.array_equal(hits["prim"], exp["prim"])
        assert same_bits(hits["u"], exp["u"]) and same_bits(hits["v"], exp["v"])
        assert same_bits(hits["t"], exp["t"] * F(tscale))


def check_window(pkg, trace):
    """The ray's own window on the dragon's hit pixels (fixture distance t0)."""
    cfg, mesh, bvh, basis, sun, meta, rec = fixture(DRAGON)
    rays_all = pkg.camera_rays(basis, cfg["W"], cfg["H"])
    hit = rec["prim"] >= 0
    rays = rays_all[rec["pixel"][hit]]
    t0 = rec["t"][hit]
    exp = np.zeros(len(rays), pkg.HIT_DTYPE)
    for k in ("prim", "t", "u", "v"):
        exp[k] = rec[k][hit]

    def run(tmin, tmax):
        r = rays.copy()
        if tmin is not None:
            r[:, 6] = tmin
        if tmax is not None:
            r[:, 7] = tmax
        h, _, _ = trace(r, 0, True, False)
        got = h["prim"] >= 0
        t, u, v = moller_trumbore(mesh, r[got], h["prim"][got])      # every reported hit is that triangle's
        assert same_bits(h["t"][got], t) and same_bits(h["u"][got], u) and same_bits(h["v"][got], v)
        assert not h["t"][~got].view(np.uint32).any()
        return r, h, got

    _, h, got = run(None, t0)                                        # inclusive upper bound
    assert hits_equal(h, exp)
    r, h, got = run(None, np.nextafter(t0, F(0)))
    assert (h["t"][got] <= r[got, 7]).all()
    r, h, got = run(np.nextafter(t0, F(np.inf)), None)
    assert (h["t"][got] >= r[got, 6]).all()
    for tmin in (F(-2), F(-np.inf)):
        r, h, got = run(tmin, None)
        assert got.all() and (h["t"] <= t0).all()
    _, h, got = run(F(0), F(0))
    assert not got.any()


@functools.lru_cache(maxsize=None)
def adversarial_rays():
    """4,099 rays against the dragon_333x217 scene, fixed seed: origins uniform in twice the root box,
    random unnormalised directions scaled by 2^k (k in [-20, 20]), one ray in eight with a component
    exactly +0 or -0, windows from tmin {0, -2, -inf, 1e-3} x tmax {FLT_MAX, +inf, 1, 0}; then the
    six axis directions from inside and from outside the box, a zero direction, NaN / +-inf in an
    origin and in a direction, and tmin > tmax.  Used for GPU-against-CPU equality, for occlusion ==
    "the closest query finds a hit", and stored with the reference's own answers as the ray set
    dragon_adversarial (tests/golden/rays/)."""
    _, _, bvh, _, _, _, _ = fixture(DRAGON)
    b = root_box(bvh).astype(np.float64)
    lo, hi = b[0::2], b[1::2]
    c, h = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(20261019)
    n = 4099
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = (c + 2 * h * rng.uniform(-1, 1, (n, 3))).astype(F)
    d = rng.normal(size=(n, 3)) * np.exp2(rng.integers(-20, 21, n))[:, None]
    rays[:, 3:6] = d.astype(F)
    eighth = np.arange(0, n, 8)
    rays[eighth, 3 + rng.integers(0, 3, len(eighth))] = np.where(rng.integers(0, 2, len(eighth)) == 1, F(-0.0), F(0.0))
    rays[:, 6] = np.asarray([0, -2, -np.inf, 1e-3], F)[rng.integers(0, 4, n)]
    rays[:, 7] = np.asarray([FLT_MAX, np.inf, 1, 0], F)[rng.integers(0, 4, n)]
    k = n - 21
    special = []
    inside = (c + 0.25 * h * rng.uniform(-1, 1, 3)).astype(F)
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = np.zeros(3, F)
            e[axis] = sign
            outside = inside.copy()
            outside[axis] = F(c[axis] - sign * 3 * h[axis])          # in front of the box, looking at it
            special.append(np.concatenate([inside, e, [0, FLT_MAX]]))
            special.append(np.concatenate([outside, e, [0, FLT_MAX]]))
    one = np.asarray([0.3, -1.0, 0.2], F)
    special.append(np.concatenate([inside, [0, 0, 0], [0, FLT_MAX]]))
    for bad in (np.nan, np.inf, -np.inf):
        o = inside.copy()
        o[1] = bad
        special.append(np.concatenate([o, one, [0, FLT_MAX]]))
        dd = one.copy()
        dd[2] = bad
        special.append(np.concatenate([inside, dd, [0, FLT_MAX]]))
    special.append(np.concatenate([inside, one, [2, 1]]))             # tmin > tmax
    special.append(np.concatenate([inside, one, [np.inf, -np.inf]]))
    assert len(special) == 21
    rays[k:] = np.asarray(special, F)
    rays.setflags(write=False)
    return rays


TINY_FIXTURES = ["tri1", "quad"]


@functools.lru_cache(maxsize=None)
def tiny_tree_rays(name):
    """357 rays (five wavefronts and a tail of 37), fixed seed, against one of the two smallest trees:
    tri1 (one triangle: the root is a leaf, the walks' root-is-leaf loop) or quad (three triangles:
    a root whose two children are leaves, one step and no stack).  Each ray is aimed from around the
    scene at a point of a triangle's plane, inside the triangle or past its edges, the direction
    scaled by 2^k (k in [-4, 4]) and reversed for one ray in four (the plane lies behind it: t < 0);
    windows from tmin {0, -2, -inf, 1e-3} x tmax {FLT_MAX, +inf, 1, 0}, the last four rays with
    tmin > tmax."""
    _, mesh, bvh, _, _, _, _ = fixture(name)
    assert (bvh.nodes[0, 6] != 0) == (name == "tri1")                 # primitive_count of the root: tri1's is a leaf
    b = root_box(bvh).astype(np.float64)
    c, h = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2
    h = np.maximum(h, h.max() / 2)                                    # a flat box still gets origins off its plane
    rng = np.random.default_rng(20261020)
    n = 357
    tr = mesh.tri.astype(np.float64)
    k = rng.integers(0, len(tr), n)
    target = tr[k, 0:3] + rng.uniform(-0.6, 1.2, (n, 1)) * tr[k, 3:6] + rng.uniform(-0.6, 1.2, (n, 1)) * tr[k, 6:9]
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = (c + 3 * h * rng.uniform(-1, 1, (n, 3))).astype(F)
    scale = np.exp2(rng.integers(-4, 5, n)) * np.where(rng.integers(0, 4, n) == 0, -1.0, 1.0)
    rays[:, 3:6] = ((target - rays[:, 0:3]) * scale[:, None]).astype(F)
    rays[:, 6] = np.asarray([0, -2, -np.inf, 1e-3], F)[rng.integers(0, 4, n)]
    rays[:, 7] = np.asarray([FLT_MAX, np.inf, 1, 0], F)[rng.integers(0, 4, n)]
    rays[-4:, 6:8] = np.asarray([[2, 1], [np.inf, -np.inf], [1e-3, 0], [1, -2]], F)
    rays.setflags(write=False)
    return rays


def check_tiny_tree_input(name, rays, hits, hits_open):
    """The conditions that keep the smallest-trees comparison from passing vacuously.  hits: the CPU
    path's closest hits of `rays`; hits_open: of the same rays under [0, FLT_MAX]."""
    _, mesh, _, _, _, _, _ = fixture(name)
    hit = hits["prim"] >= 0
    assert hit.any() and (~hit).any(), name
    assert ((hits_open["prim"] >= 0) & ~hit).any(), name             # the ray's own window rejects a hit
    # a missing ray with tmin <= -1 and a failed u, v or w stage on some triangle: a fail mark of -1
    # would pass its window
    cand = ~hit & (rays[:, 6] <= -1) & (rays[:, 7] >= -1)
    failed = np.zeros(len(rays), bool)
    for p in range(len(mesh)):
        _, u, v = moller_trumbore(mesh, rays, np.full(len(rays), p))
        with np.errstate(invalid="ignore"):
            failed |= (u < 0) | (v < 0) | (F(1) - u - v < 0)
    assert (cand & failed).any(), name


def modes(pkg):
    """{exact, FMA} x {fast, robust}: (mode, scene-prep arithmetic)."""
    return [(0, pkg.ARITH_EXACT), (pkg.MODE_ROBUST, pkg.ARITH_EXACT), (pkg.MODE_FMA, pkg.ARITH_FMA),
            (pkg.MODE_FMA | pkg.MODE_ROBUST, pkg.ARITH_FMA)]


# ---------------------------------------------------------------- rays the reference traced itself
# tests/golden/rays/<set>.npz (tests/golden/make_golden_rays.py): caller-style rays and what the
# reference's own traverser.traverse(ray, intersector, statistics) returned for each, from its four
# builds.  The sets and the kernel paths they reach are listed in DESIGN.md (ray queries, Tests).

RAY_SETS = ["dragon_adversarial", "dragon_octants", "tri1_tiny", "quad_tiny", "proc300_window", "lattice_ties",
            "arms6_centroids", "bodyarms_centroids"]
RAY_VARIANTS = ["exact_fast", "exact_robust", "ref_fast", "ref_robust"]
RAY_FIELDS = ("prim", "t", "u", "v", "occluded", "steps", "tests")
RAYS_DIR = os.path.join(GOLDEN, "rays")
WINDOW_TMIN = np.asarray([0, -2, -np.inf, 1e-3], F)
WINDOW_TMAX = np.asarray([FLT_MAX, np.inf, 1, 0], F)

# dragon_octants: 24 uniform groups (octant g // 3), one group uniform but for a lane, a tail of 37
OCT_GROUPS, OCT_MIXED, OCT_TAIL = 24, (5, 2, 17), (3, 37)           # (octant, the odd lane's octant, the lane); (octant, rays)
OCT_N = 64 * (OCT_GROUPS + 1) + OCT_TAIL[1]
# the eight specials, one inside a uniform group of each octant: (group, lane, tmin, tmax, aimed to hit)
_NAN = float("nan")
OCT_SPECIALS = [(0, 5, _NAN, None, False), (4, 14, None, _NAN, False), (8, 23, _NAN, _NAN, False),
                (9, 33, _NAN, None, True), (13, 42, None, _NAN, True), (17, 51, _NAN, _NAN, True),
                (18, 60, np.inf, None, True), (22, 9, None, -np.inf, True)]


def variant_mode(pkg, variant):
    """(mode, scene-prep arithmetic) of a reference build x traverser."""
    return dict(zip(RAY_VARIANTS, modes(pkg)))[variant]


def ray_octant(rays):
    """The octant the fast walk dispatches on: bit a is the sign bit of safe_inverse(d[a])
    (vector.hpp:69-74 keeps the sign of d, of +-0 too), so -0 counts as negative."""
    s = np.signbit(rays[:, 3:6])
    return s[:, 0] | s[:, 1] << 1 | s[:, 2] << 2


@functools.lru_cache(maxsize=None)
def octant_rays():
    """1,637 rays against the dragon_333x217 scene, fixed seed, laid out in wavefronts of 64
    consecutive rays: for each octant three groups whose directions all carry its signs; then a
    group of octant 5 with lane 17 of octant 2; then a tail of 37 rays of octant 3.  Half the rays
    are aimed at a triangle's centroid, the others at a point of the root box, from an origin up to
    2.5 half-extents away on the octant's side (around and inside the box); the direction is
    (target - origin) * 2^k, k in [-20, 20]; windows from the adversarial table.  One ray in eight
    has a component exactly zero, signed to stay in its group's octant, and its origin moved so the
    ray still passes its target.  Eight specials sit inside uniform groups (OCT_SPECIALS): NaN as
    tmin, as tmax and as both, on any ray and on a ray aimed to hit, then tmin = +inf and
    tmax = -inf."""
    _, mesh, bvh, _, _, _, _ = fixture(DRAGON)
    b = root_box(bvh).astype(np.float64)
    c, h = (b[0::2] + b[1::2]) / 2, (b[1::2] - b[0::2]) / 2
    rng = np.random.default_rng(20261021)
    n = OCT_N
    octant = np.repeat(np.arange(OCT_GROUPS + 2) // 3, 64)[:n]
    octant[64 * OCT_GROUPS:64 * (OCT_GROUPS + 1)] = OCT_MIXED[0]
    octant[64 * OCT_GROUPS + OCT_MIXED[2]] = OCT_MIXED[1]
    octant[64 * (OCT_GROUPS + 1):] = OCT_TAIL[0]
    sign = np.where((octant[:, None] >> np.arange(3)) & 1, -1.0, 1.0)
    aimed = rng.integers(0, 2, n) == 1
    special = {64 * g + lane: (tmin, tmax) for g, lane, tmin, tmax, _ in OCT_SPECIALS}
    for g, lane, _, _, hit in OCT_SPECIALS:
        aimed[64 * g + lane] |= hit
    tr = mesh.tri[rng.integers(0, len(mesh), n)].astype(np.float64)
    centroid = tr[:, 0:3] + (tr[:, 6:9] - tr[:, 3:6]) / 3             # p0, p0 - e1, p0 + e2
    target = np.where(aimed[:, None], centroid, c + h * rng.uniform(-1, 1, (n, 3)))
    origin = (target - sign * h * rng.uniform(0.05, 2.5, (n, 3))).astype(F)
    zero = np.zeros(n, bool)
    zero[0::8] = True
    axis = rng.integers(0, 3, n)
    origin[zero, axis[zero]] = target[zero, axis[zero]].astype(F)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = origin
    d = (target - origin) * np.exp2(rng.integers(-20, 21, n))[:, None]
    d[zero, axis[zero]] = 0
    rays[:, 3:6] = np.copysign(d, sign).astype(F)
    rays[:, 6] = WINDOW_TMIN[rng.integers(0, 4, n)]
    rays[:, 7] = WINDOW_TMAX[rng.integers(0, 4, n)]
    for k, (tmin, tmax) in special.items():
        assert not zero[k]
        rays[k, 6:8] = (0, FLT_MAX) if aimed[k] else rays[k, 6:8]     # open, but for the special bound
        if tmin is not None:
            rays[k, 6] = tmin
        if tmax is not None:
            rays[k, 7] = tmax
    assert np.array_equal(ray_octant(rays), octant) and (rays[:, 3:6] != 0).any(axis=1).all()
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def proc300(arith=0):
    """(cfg, mesh, bvh, camera) of the 300 x 300 heightfield under proc_101's camera: about 94,000
    sibling pairs, node indices past 16 bits (the walks' 24-bit stack planes)."""
    pkg = import_package()
    cfg = dict(pkg.configs.CONFIGS["proc_101"])
    cfg["proc"] = 300
    return (cfg,) + tuple(pkg.prepare(cfg, arith=arith))


@functools.lru_cache(maxsize=None)
def proc300_window_rays():
    """The rays of test_gpu_equals_cpu_with_24_bit_stack_entries (exact arithmetic: the camera rays in
    reverse order without the last 13, windows by k % 4 and (k // 4) % 4), thinned to every ray whose
    index is a multiple of 4 plus the last 51 -- which carry all 16 windows."""
    pkg = import_package()
    cfg, _, _, cam = proc300(0)
    rays = np.ascontiguousarray(pkg.camera_rays(cam.basis(cfg["W"], cfg["H"]), cfg["W"], cfg["H"])[::-1][:-13])
    k = np.arange(len(rays))
    rays[:, 6] = WINDOW_TMIN[k % 4]
    rays[:, 7] = WINDOW_TMAX[(k // 4) % 4]
    keep = (k % 4 == 0) | (k >= len(rays) - 51)
    rays = np.ascontiguousarray(rays[keep])
    rays.setflags(write=False)
    return rays

# ---------------------------------------------------------------- the lattice: exact ties
# 128 unit right triangles on the integer grid (4 x 4 cells, two triangles each) in the layers z = 0,
# 1, 2 and a coincident copy of the z = 0 layer whose zeros are written "-0".  Rays from the
# half-integer grid with direction components and windows that are small dyadic numbers: every
# product, sum and quotient of a triangle or slab test is exact in float (and in double), so u, v,
# w = 0, t = tmin, t = tmax and equal t on two triangles occur by the hundred, and FMA contraction
# has nothing to change.
LATTICE = "lattice_ties"
LATTICE_OBJ = os.path.join(GOLDEN, "lattice.obj")
LATTICE_CELLS = 4
LATTICE_LAYERS = ("0", "1", "2", "-0")                                # the last: the coincident copy of the first
LATTICE_N = 4096
LATTICE_DIRS = np.asarray([0.0, -0.0, 0.5, -0.5, 1, -1, 2, -2], F)
LATTICE_TMIN = np.asarray([0, 0.5, 1, 2, -2, -np.inf], F)
LATTICE_TMAX = np.asarray([0.5, 1, 2, 3, 4, FLT_MAX, np.inf], F)


def lattice_obj_text():
    """tests/golden/lattice.obj: per layer 25 vertices (coordinate strings: the integers, and "-0" for
    every zero of the copy layer) and 32 faces, the two triangles of a cell split along alternating
    diagonals and wound alternately, so that edges, diagonals and vertices all lie on rays' paths."""
    n = LATTICE_CELLS
    out = ["# %d unit right triangles on the integer grid: layers z = 0, 1, 2 and a copy of z = 0 written with -0"
           % (2 * n * n * len(LATTICE_LAYERS))]
    for layer, z in enumerate(LATTICE_LAYERS):
        neg = z.startswith("-")
        for j in range(n + 1):
            for i in range(n + 1):
                out.append("v %s %s %s" % ("-0" if neg and i == 0 else i, "-0" if neg and j == 0 else j, z))
        base = layer * (n + 1) * (n + 1) + 1
        for j in range(n):
            for i in range(n):
                a = base + j * (n + 1) + i
                b, c, d = a + 1, a + n + 2, a + n + 1
                tris = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
                for k, t in enumerate(tris):
                    if (i + j + k + layer) % 3 == 0:                   # a third wound the other way
                        t = (t[0], t[2], t[1])
                    out.append("f %d %d %d" % t)
    return "\n".join(out) + "\n"


def lattice_twins():
    """The triangles that have a coincident twin: the z = 0 layer and its copy."""
    per = 2 * LATTICE_CELLS * LATTICE_CELLS
    return np.concatenate([np.arange(per), np.arange(3 * per, 4 * per)])


@functools.lru_cache(maxsize=None)
def lattice(arith=0):
    """(cfg, mesh, bvh) of the lattice under quad's camera (unused: no frame of it is rendered)."""
    pkg = import_package()
    cfg = dict(pkg.configs.CONFIGS["quad"], obj="@golden/lattice.obj")
    mesh, bvh, _ = pkg.prepare(cfg, arith=arith)
    return cfg, mesh, bvh


@functools.lru_cache(maxsize=None)
def lattice_rays():
    """4,096 rays, fixed seed: origins on the half-integer grid, x, y in [-1, 5] and z from {-1,
    -0.5, -0, 0, 0.5, ..., 3} (the layer heights and both zeros included); direction components from
    {+0, -0, +-0.5, +-1, +-2}, the all-zero directions kept; windows from {0, 0.5, 1, 2, -2, -inf} x
    {0.5, 1, 2, 3, 4, FLT_MAX, +inf}.  Stored order is shuffled until no wavefront of 64 consecutive
    rays is uniform in its octant (the generic loop); sorted by octant (lattice_octant_order) most
    wavefronts are (the kOct 0..7 loops)."""
    rng = np.random.default_rng(20261023)
    n = LATTICE_N
    rays = np.zeros((n, 8), F)
    rays[:, 0:2] = (rng.integers(-2, 11, (n, 2)) * 0.5).astype(F)
    z = np.asarray([-1, -0.5, -0.0, 0.0, 0.5, 1, 1.5, 2, 2.5, 3], F)
    rays[:, 2] = z[rng.integers(0, len(z), n)]
    rays[:, 3:6] = LATTICE_DIRS[rng.integers(0, len(LATTICE_DIRS), (n, 3))]
    rays[:, 6] = LATTICE_TMIN[rng.integers(0, len(LATTICE_TMIN), n)]
    rays[:, 7] = LATTICE_TMAX[rng.integers(0, len(LATTICE_TMAX), n)]
    while any(len(set(ray_octant(rays[k:k + 64]).tolist())) == 1 for k in range(0, n, 64)):
        rays = rays[rng.permutation(n)]
    rays = np.ascontiguousarray(rays)
    rays.setflags(write=False)
    return rays


def lattice_octant_order(rays):
    """A stable argsort by octant: each octant's rays become consecutive, in stored order."""
    return np.argsort(ray_octant(rays), kind="stable")


def uniform_wavefronts(octant):
    """Per octant, the number of whole wavefronts (64 consecutive rays from a multiple of 64) that hold
    that octant alone."""
    count = np.zeros(8, np.int64)
    for k in range(0, len(octant) - 63, 64):
        w = octant[k:k + 64]
        if (w == w[0]).all():
            count[w[0]] += 1
    return count



# ---------------------------------------------------------------- deep trees: rays at every level
# arms6_centroids / bodyarms_centroids (tests/deep_common.py: BVHs of 52 and 53 levels; the
# nearest-first BVH4 bound, which sizes the query kernels' LDS, 61 and 67).
DEEP_SETS = {"arms6_centroids": "arms6_zoom20", "bodyarms_centroids": "bodyarms_wide"}
DEEP_SPECIALS = [(0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf), (6, np.nan), (7, np.nan)]


@functools.lru_cache(maxsize=None)
def centroid_rays(name):
    """Four rays per triangle, fixed seed, each aimed at the triangle's centroid c from c + r e (e a
    random unit vector): r = 3 |c| (the triangle's own level of the tree), r = 3 x 2^10 |c| (ten
    levels up) and r = 3 x 2^30 (outside the largest triangle: the whole chain of boxes lies on the
    ray's way), and a fourth from 3 |c| with the direction reversed, so the triangle lies behind it.
    Directions are target - origin as rounded (the centroid at t ~ 1); windows from the adversarial
    table, so tmax = 1 ends at the aimed triangle, give or take the rounding.  In every wavefront of
    64 consecutive rays one ray gets a non-finite float (DEEP_SPECIALS in turn: the float's index in
    the ray, the value), at lane 7 x wavefront mod 64."""
    _, mesh, _, _, _, _, _ = fixture(DEEP_SETS[name])
    tr = mesh.tri.astype(np.float64)
    c = tr[:, 0:3] + (tr[:, 6:9] - tr[:, 3:6]) / 3                    # p0, p0 - e1, p0 + e2
    n = 4 * len(tr)
    rng = np.random.default_rng(20261024)
    e = rng.normal(size=(n, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    size = np.repeat(np.linalg.norm(c, axis=1), 4)
    r = 3.0 * np.where(np.arange(n) % 4 == 1, size * 2.0 ** 10, np.where(np.arange(n) % 4 == 2, 2.0 ** 30, size))
    target = np.repeat(c, 4, axis=0)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = (target + r[:, None] * e).astype(F)
    d = target - rays[:, 0:3]
    d[3::4] *= -1.0
    rays[:, 3:6] = d.astype(F)
    rays[:, 6] = WINDOW_TMIN[rng.integers(0, 4, n)]
    rays[:, 7] = WINDOW_TMAX[rng.integers(0, 4, n)]
    for w in range((n + 63) // 64):
        k = 64 * w + 7 * w % 64
        if k < n:
            col, value = DEEP_SPECIALS[w % len(DEEP_SPECIALS)]
            rays[k, col] = value
    rays.setflags(write=False)
    return rays


_SET_CONFIG = dict({"dragon_adversarial": DRAGON, "dragon_octants": DRAGON, "tri1_tiny": "tri1", "quad_tiny": "quad"}, **DEEP_SETS)


def ray_set_rays(name):
    """The generator of a set's rays (the fixture stores its output)."""
    if name in DEEP_SETS:
        return centroid_rays(name)
    return {"dragon_adversarial": adversarial_rays, "dragon_octants": octant_rays, "proc300_window": proc300_window_rays,
            "tri1_tiny": lambda: tiny_tree_rays("tri1"), "quad_tiny": lambda: tiny_tree_rays("quad"), LATTICE: lattice_rays}[name]()


def ray_set_config(name):
    """The config whose scene a set's rays are traced against."""
    pkg = import_package()
    if name == "proc300_window":
        return proc300(0)[0]
    if name == LATTICE:
        return lattice(0)[0]
    return pkg.configs.CONFIGS[_SET_CONFIG[name]]


def ray_set_scene(name, arith=0):
    """(mesh, bvh) of a set's scene, prepared in the given arithmetic."""
    if name == "proc300_window":
        return proc300(arith)[1:3]
    if name == LATTICE:
        return lattice(arith)[1:3]
    return fixture(_SET_CONFIG[name], arith)[1:3]


@functools.lru_cache(maxsize=None)
def load_ray_fixture(name):
    """tests/golden/rays/<name>.npz: {"rays": float32 [n, 8], variant: {prim, t, u, v (uint32 bits),
    occluded, steps, tests}}; read-only arrays, loaded once."""
    z = np.load(os.path.join(RAYS_DIR, name + ".npz"))
    out = {"rays": z["rays"]}
    for v in RAY_VARIANTS:
        out[v] = {k: z[v + "_" + k] for k in RAY_FIELDS}
    for a in [out["rays"]] + [a for v in RAY_VARIANTS for a in out[v].values()]:
        a.setflags(write=False)
    assert out["rays"].dtype == F and out["rays"].shape[1] == 8
    return out


def reference_hits(pkg, ref):
    """A variant's records as the API's hit16 array {prim, t, u, v}."""
    exp = np.zeros(len(ref["prim"]), pkg.HIT_DTYPE)
    exp["prim"] = ref["prim"]
    for k in ("t", "u", "v"):
        exp[k] = ref[k].view(F)
    return exp


def check_against_ray_fixture(pkg, trace, name, variant, stats, closest=True, occluded=True, select=None):
    """trace(rays, mode, closest, occluded) on the set's scene prepared for `variant` must return the
    reference's own answer for every stored ray (select: an index array, for a reordered or shortened
    run): prim equal, t, u, v bit for bit, misses {-1, 0, 0, 0}, occluded equal; counters rays = n
    and hits = the reference's hit count.  stats (the CPU path, GPU stats scenes): the rays none of
    whose eight floats is NaN go in one call, the others in a call of their own, and each call's
    node_pairs / tri_tests are the sums of the reference's traversal_steps / intersections of the
    closest walk over its rays.  Otherwise one call in stored order, so that the wavefronts are the
    ones the set lays out."""
    fx = load_ray_fixture(name)
    ref = fx[variant]
    mode, _ = variant_mode(pkg, variant)
    exp_h, exp_o = reference_hits(pkg, ref), ref["occluded"].astype(np.uint8)
    miss = exp_h["prim"] < 0
    assert not exp_h["t"][miss].view(np.uint32).any() and not exp_h["u"][miss].view(np.uint32).any()
    assert not exp_h["v"][miss].view(np.uint32).any() and (exp_h["prim"] >= -1).all()
    idx = np.arange(len(fx["rays"])) if select is None else np.asarray(select)
    parts = [idx]
    if stats:
        nan = np.isnan(fx["rays"][idx]).any(axis=1)
        parts = [idx[~nan]] + ([idx[nan]] if nan.any() else [])
    for k, part in enumerate(parts):
        rays = np.ascontiguousarray(fx["rays"][part])
        hits, occ, st = trace(rays, mode, closest, occluded)
        where = (name, variant, "stats" if stats else "production", "part %d" % k)
        if closest:
            bad = np.flatnonzero(hits.view(np.uint32).reshape(-1, 4) != exp_h[part].view(np.uint32).reshape(-1, 4))
            assert hits.tobytes() == exp_h[part].tobytes(), (where, "first differing ray", int(part[bad[0] // 4]), len(bad))
        if occluded:
            assert np.array_equal(occ, exp_o[part]), (where, np.flatnonzero(occ != exp_o[part])[:8])
        assert st["rays"] == len(part), where
        assert st["hits"] == int((~miss[part]).sum() if closest else exp_o[part].sum()), where
        if stats and closest:
            assert st["node_pairs"] == int(ref["steps"][part].sum(dtype=np.uint64)), where
            assert st["tri_tests"] == int(ref["tests"][part].sum(dtype=np.uint64)), where


def lattice_tie_counts(rays, ref):
    """How often the lattice set meets each boundary in one variant's stored records (rays and the
    viewed t, u, v in the set's own precision): hits, u == 0, v == 0, 1 - u - v == 0, t == tmin,
    t == tmax, a negative-zero u or v, a hit on a triangle with a coincident twin."""
    real = rays.dtype.type
    hit = ref["prim"] >= 0
    t, u, v = (ref[k].view(real) for k in ("t", "u", "v"))
    w = real(1) - u - v                                               # triangle.hpp:107, exact here
    return {"hits": int(hit.sum()), "u0": int((hit & (u == 0)).sum()), "v0": int((hit & (v == 0)).sum()),
            "w0": int((hit & (w == 0)).sum()), "tmin": int((hit & (t == rays[:, 6])).sum()),
            "tmax": int((hit & (t == rays[:, 7])).sum()),
            "neg0": int((hit & (((u == 0) & np.signbit(u)) | ((v == 0) & np.signbit(v)))).sum()),
            "twin": int((hit & np.isin(ref["prim"], lattice_twins())).sum())}


def check_lattice_conditions(fx, robust=True):
    """The floors the reference's own answers to the lattice set must meet for the comparison to test
    the boundaries (asserted by the generator and by a CPU test, on the stored outputs alone).  fx:
    load_ray_fixture(LATTICE) or its double counterpart (robust=False: no robust variants there)."""
    rays = fx["rays"]
    assert len(rays) == LATTICE_N and not np.isnan(rays).any()
    assert int((rays[:, 3:6] == 0).all(axis=1).sum()) >= 4            # all-zero directions stay in
    c = lattice_tie_counts(rays, fx["exact_fast"])
    assert min(c["u0"], c["v0"], c["w0"]) >= 50, c
    assert c["tmin"] >= 20 and c["tmax"] >= 20 and c["neg0"] >= 20 and c["twin"] >= 50, c
    fields = ("prim", "t", "u", "v", "occluded", "steps", "tests")
    for kind in ("fast", "robust") if robust else ("fast",):        # nothing for contraction to change
        a, b = fx["exact_" + kind], fx["ref_" + kind]
        for k in fields:
            assert np.array_equal(a[k], b[k]), (kind, k)
    if robust:
        a, b = fx["exact_fast"], fx["exact_robust"]
        differ = np.any([a[k] != b[k] for k in ("prim", "t", "u", "v", "occluded")], axis=0)
        assert differ.sum() >= 100, int(differ.sum())
    octant = ray_octant(rays)
    assert not uniform_wavefronts(octant).any()                       # stored order: the generic loop
    assert (uniform_wavefronts(octant[lattice_octant_order(rays)]) >= 4).all()
    return c


def check_ray_fixture_conditions(pkg, cpu_scene_of):
    """What keeps the fixture comparisons from passing vacuously, asserted on the stored reference
    outputs.  cpu_scene_of(set, arith) -> a CpuScene, used only to open windows."""
    fx = load_ray_fixture("dragon_octants")
    rays, ref = fx["rays"], fx["exact_fast"]
    hit = ref["prim"] >= 0
    octant = ray_octant(rays)
    uniform = np.arange(len(rays)) < 64 * OCT_GROUPS
    for o in range(8):
        g = uniform & (octant == o)
        assert g.sum() == 192 and (hit & g).sum() >= 10 and (~hit & g).sum() >= 10, o
    assert (hit & (rays[:, 3:6] == 0).any(axis=1)).any()
    open_rays = np.array(rays)
    open_rays[:, 6:8] = (0, FLT_MAX)
    open_hit = cpu_scene_of("dragon_octants", 0).trace(open_rays, mode=0, closest=True)[0]["prim"] >= 0
    assert (open_hit & ~hit).any()                                    # the ray's own window rejects a hit
    for g, lane, tmin, tmax, aimed in OCT_SPECIALS:
        k = 64 * g + lane
        assert k < 64 * OCT_GROUPS and not hit[k], k                  # inside a uniform group; no window with a NaN,
        if aimed:                                                     # tmin = +inf or tmax = -inf admits a hit
            assert open_hit[k], k                                     # ... though the ray would hit
    assert np.isnan(rays[:, 6:8]).any(axis=1).sum() == 6
    differ = 0
    for name in RAY_SETS:
        f = load_ray_fixture(name)
        for build in ("exact", "ref"):
            a, b = f[build + "_fast"], f[build + "_robust"]
            differ += int(np.any([a[k] != b[k] for k in ("prim", "t", "u", "v", "occluded")], axis=0).sum())
    assert differ > 0
