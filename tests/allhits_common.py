"""Shared pieces of the all-hits ray-query tests (test_allhits_cpu.py, test_gpu_allhits.py).

The hit set of a ray is what the reference's SingleRayTraverser::traverse presents to an intersector
that never lowers ray.tmax: the BVH2 walk of single_ray_traverser.hpp:68-126 with every box test and
every triangle test against the ray's original [tmin, tmax].  model() below is that walk in Python over
the reference-layout nodes (bvh.nodes, bvh.prim) -- the FastNodeIntersector in contraction-free float32,
its fma rounded once from the exact value -- and the checks every path must pass, each taking a
`trace_all(rays, max_hits, mode, hits) -> (counts, rows | None, stats)` callable.

The second half holds the reference's own answer: the sets, the loader and the comparison for
tests/golden/rays_all/ (the reference's traverser run with a collecting intersector, all four variants),
which pin the CPU path and the GPU alike; the model above stays as the exact_fast cross-check that needs no
reference build."""
import functools
import hashlib
import os
import types
from fractions import Fraction

import numpy as np

import soup_common
import trace_common as tc
from conftest import GOLDEN, import_package
from refit_common import node_fields

F = np.float32
MAX_HITS = 32
EPS = F(np.finfo(np.float32).eps)
MODEL_SETS = {"lattice_ties": None, "quad_tiny": None, "tri1_tiny": None, "dragon_adversarial": 512}   # set -> first n rays
PREFIX_K = (1, 2, 5, 8)


# ---------------------------------------------------------------- float32 fma, rounded once

def _round_f32(q):
    """The float32 nearest a non-zero Fraction (ties to even, gradual underflow, overflow to inf)."""
    neg, q = q < 0, abs(q)
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()                               # 2^e <= q < 2^(e + 1), after the fix-up
    if (n << -e if e < 0 else n) < (d << e if e > 0 else d):
        e -= 1
    ue = max(e, -126) - 23                                            # the exponent of an ulp at q
    num, den = (n << -ue, d) if ue < 0 else (n, d << ue)
    m, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and m & 1):
        m += 1
    x = float(m) * 2.0 ** ue if ue > -1000 else 0.0
    with np.errstate(over="ignore"):
        return F(-x if neg else x)                                    # m < 2^25: exact in double; >= 2^128 becomes inf


def fma32(a, b, c):
    """fma(a, b, c) in float32: the exact a b + c rounded once (never through double)."""
    a, b, c = float(a), float(b), float(c)
    p = a * b                                                         # exact in double (24 x 24 bits) or non-finite
    s = p + c
    if not np.isfinite(s) or not np.isfinite(p):
        with np.errstate(all="ignore"):
            return F(s)                                               # an inf or NaN operand: the sum's inf / NaN
    bb = s - p
    if (p - (s - bb)) + (c - bb) == 0.0:                              # TwoSum: the double sum is exact, one rounding follows
        with np.errstate(over="ignore"):
            return F(s)
    return _round_f32(Fraction(a) * Fraction(b) + Fraction(c))


# ---------------------------------------------------------------- the model

def _accept(mesh, ray, prims):
    """Triangle::intersect of one ray on the triangles `prims` (original indices): (accepted mask, t, u, v)."""
    r = np.broadcast_to(ray, (len(prims), 8))
    t, u, v = tc.moller_trumbore(mesh, r, prims)
    with np.errstate(invalid="ignore"):
        ok = (u >= 0) & (v >= 0) & (F(1) - u - v >= 0) & (t >= ray[6]) & (t <= ray[7])
    return ok, t, u, v


def model_ray(mesh, bvh, ray):
    """(hits sorted by the key as (t, prim, u, v) tuples, traversal steps, tested triangles) of one ray:
    the fixed-window walk with the FastNodeIntersector (node_intersectors.hpp:35-47,83-103)."""
    bounds, count, first = node_fields(bvh.nodes)
    prim = np.asarray(bvh.prim, np.int64)
    tmin, tmax = ray[6], ray[7]
    found, steps, tests = [], 0, 0

    def leaf(k):
        nonlocal tests
        p = prim[first[k]:first[k] + count[k]]
        tests += len(p)
        ok, t, u, v = _accept(mesh, ray, p)
        found.extend((t[j], int(p[j]), u[j], v[j]) for j in np.flatnonzero(ok))

    if count[0]:
        leaf(0)
    else:
        with np.errstate(all="ignore"):
            d = ray[3:6]
            inv = F(1) / np.where(np.abs(d) < EPS, np.copysign(EPS, d), d).astype(F)     # safe_inverse, vector.hpp:69-74
            so = (-ray[0:3]) * inv
        octant = np.signbit(d).astype(int)

        def box(k):
            b = bounds[k]
            e = [fma32(b[2 * a + octant[a]], inv[a], so[a]) for a in range(3)]
            x = [fma32(b[2 * a + 1 - octant[a]], inv[a], so[a]) for a in range(3)]
            gt = lambda p, q: p if p > q else q                      # noqa: E731  robust_max: the right operand unless p > q
            lt = lambda p, q: p if p < q else q                      # noqa: E731  robust_min
            return gt(e[0], gt(e[1], gt(e[2], tmin))) <= lt(x[0], lt(x[1], lt(x[2], tmax)))

        stack, left = [], first[0]
        while True:
            steps += 1
            go = []
            for k in (left, left + 1):
                if box(k):
                    if count[k]:
                        leaf(k)
                    else:
                        go.append(k)
            if len(go) == 2:
                stack.append(first[go[1]])
            if go:
                left = first[go[0]]
            elif stack:
                left = stack.pop()
            else:
                break
    # the key: t ascending by float <, equal t (-0 == +0) by original triangle index
    found.sort(key=lambda h: (float(h[0]), h[1]))
    return found, steps, tests


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's answer to the set's (first MODEL_SETS[name]) rays in the exact_fast variant:
    (counts [n] u32, rows [n, 32] HIT_DTYPE, steps, tests), computed once."""
    pkg = import_package()
    mesh, bvh = tc.ray_set_scene(name, 0)
    rays = tc.load_ray_fixture(name)["rays"][:MODEL_SETS[name]]
    counts = np.zeros(len(rays), np.uint32)
    rows = np.zeros((len(rays), MAX_HITS), pkg.HIT_DTYPE)
    rows["prim"] = -1
    steps = tests = 0
    for k, ray in enumerate(rays):
        found, s, t = model_ray(mesh, bvh, ray)
        steps, tests = steps + s, tests + t
        counts[k] = len(found)
        for i, (ht, hp, hu, hv) in enumerate(found[:MAX_HITS]):
            rows[k, i] = (hp, ht, hu, hv)
    for a in (counts, rows):
        a.setflags(write=False)
    return counts, rows, steps, tests


def brute_force_counts(name):
    """Per ray, how many of ALL the scene's triangles pass Triangle::intersect in the ray's window (small
    scenes only): NOT the definition of the hit set -- the walk tests a triangle only behind its boxes."""
    mesh, _ = tc.ray_set_scene(name, 0)
    rays = tc.load_ray_fixture(name)["rays"]
    n = np.zeros(len(rays), np.int64)
    for p in range(len(mesh)):
        t, u, v = tc.moller_trumbore(mesh, rays, np.full(len(rays), p))
        with np.errstate(invalid="ignore"):
            n += (u >= 0) & (v >= 0) & (F(1) - u - v >= 0) & (t >= rays[:, 6]) & (t <= rays[:, 7])
    return n


# ---------------------------------------------------------------- the checks

def rows_equal(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_reference_answers(pkg, trace_all, name, variant):
    """What follows from the closest walk's window only ever shrinking, against the reference's stored
    answers (tests/golden/rays/): count >= 1 exactly where the reference's occluded is 1; the reference's
    closest hit is one of the listed records, bit for bit, where count <= 32; the first listed t is <= the
    reference's t; stats.hits is the reference's occluded count."""
    fx = tc.load_ray_fixture(name)
    ref = fx[variant]
    mode, _ = tc.variant_mode(pkg, variant)
    counts, rows, st = trace_all(fx["rays"], MAX_HITS, mode, True)
    occ = ref["occluded"].astype(bool)
    assert np.array_equal(counts >= 1, occ), (name, variant, np.flatnonzero((counts >= 1) != occ)[:8])
    assert st["rays"] == len(fx["rays"]) and st["hits"] == int(occ.sum()), (name, variant)
    exp = tc.reference_hits(pkg, ref)
    hit = exp["prim"] >= 0
    assert np.array_equal(hit, occ)
    listed = hit & (counts <= MAX_HITS)
    same = (rows.view(np.uint32).reshape(len(rows), MAX_HITS, 4) == exp.view(np.uint32).reshape(-1, 1, 4)).all(axis=2).any(axis=1)
    assert same[listed].all(), (name, variant, np.flatnonzero(listed & ~same)[:8])
    assert (rows["t"][hit, 0] <= exp["t"][hit]).all(), (name, variant)
    return counts, rows


def check_rows(rays, counts, rows, K):
    """A [n, K] answer is well formed: rows sorted by the key, prims distinct, every t inside the ray's
    window, min(count, K) records then misses that are all-zero after prim = -1."""
    n = len(rays)
    assert counts.shape == (n,) and counts.dtype == np.uint32 and rows.shape == (n, K)
    kept = np.minimum(counts, K).astype(np.int64)
    slot = np.arange(K)[None, :]
    real = slot < kept[:, None]
    assert np.array_equal(rows["prim"] >= 0, real)
    miss = rows[~real]
    assert (miss["prim"] == -1).all() and not miss["t"].view(np.uint32).any()
    assert not miss["u"].view(np.uint32).any() and not miss["v"].view(np.uint32).any()
    t, p = rows["t"], rows["prim"]
    assert not np.isnan(t[real]).any()
    assert ((t >= rays[:, 6:7]) & (t <= rays[:, 7:8]))[real].all()
    pair = real[:, 1:]                                                # slots i, i + 1 both real
    a, b, pa, pb = t[:, :-1], t[:, 1:], p[:, :-1], p[:, 1:]
    assert ((a < b) | ((a == b) & (pa < pb)))[pair].all()             # strictly increasing key: prims distinct too
    for k in np.flatnonzero(kept > 1):                                # ... distinct across the whole row, said directly
        assert len(set(p[k, :kept[k]].tolist())) == kept[k]


def check_list_properties(trace_all, rays, mode):
    """check_rows at max_hits = 32; the row for K equals the first K records of the 32-row (K in 1, 2, 5,
    8) and counts are identical for every K and for the count-only call; a permutation of the rays
    permutes the answers.  Returns (counts, rows at 32)."""
    rays = np.ascontiguousarray(rays)
    counts, rows, st = trace_all(rays, MAX_HITS, mode, True)
    check_rows(rays, counts, rows, MAX_HITS)
    assert st["rays"] == len(rays) and st["hits"] == int((counts >= 1).sum())
    for K in PREFIX_K:
        c, r, _ = trace_all(rays, K, mode, True)
        assert np.array_equal(c, counts), K
        assert rows_equal(r, np.ascontiguousarray(rows[:, :K])), K
    c, r, st0 = trace_all(rays, 0, mode, False)
    assert r is None and np.array_equal(c, counts) and st0["hits"] == st["hits"]
    perm = np.random.default_rng(20261025).permutation(len(rays))
    c, r, _ = trace_all(rays[perm], MAX_HITS, mode, True)
    assert np.array_equal(c, counts[perm]) and rows_equal(r, np.ascontiguousarray(rows[perm]))
    return counts, rows


def rows_with_equal_t(counts, rows):
    """Per ray: does its row hold two records with equal t (adjacent, since the row is sorted)."""
    kept = np.minimum(counts, rows.shape[1]).astype(np.int64)
    pair = np.arange(1, rows.shape[1])[None, :] < kept[:, None]
    return ((rows["t"][:, :-1] == rows["t"][:, 1:]) & pair).any(axis=1)


# ---------------------------------------------------------------- rays the reference collected itself
# tests/golden/rays_all/<set>.npz (tests/golden/make_golden_allhits.py): what the reference's own
# traverser.traverse(ray, intersector, statistics) presented to a collecting intersector that never lowers
# ray.tmax (oracle/ref_harness.cpp --ray-all-hits), in the four variants of tc.RAY_VARIANTS: for the eight
# sets of tc.RAY_SETS, whose rays stay in tests/golden/rays/ (the file holds their sha256), and for the sets
# below, whose rays it stores.

ALL_DIR = os.path.join(GOLDEN, "rays_all")
DUPLEAF = "dupleaf_stack"
SOUP_SETS = {"soup_%s_%d" % c: c for c in soup_common.RENDERED}
NEW_SETS = [DUPLEAF] + list(SOUP_SETS)
ALL_SETS = tc.RAY_SETS + NEW_SETS
HIT_FIELDS = ("prim", "t", "u", "v")
HIT_DTYPE = np.dtype([("prim", np.int32), ("t", F), ("u", F), ("v", F)])   # the package's (asserted by test_allhits_cpu.py)
DUPLEAF_OBJ = os.path.join(GOLDEN, "dupleaf.obj")
SOUP_RAYS, SOUP_RADIUS, SOUP_SPECIALS = 1024, 12.0, 8


def _tri_rows(p):
    """bvh::Triangle<float> rows {p0, e1 = p0 - p1, e2 = p2 - p0, n = cross(e1, e2)} of [n, 3, 3] float32
    vertices, contraction-free (triangle.hpp:27-30)."""
    p0, e1, e2 = p[:, 0], p[:, 0] - p[:, 1], p[:, 2] - p[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return np.concatenate([p0, e1, e2, n], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def dupleaf_stacks():
    """tests/golden/dupleaf.obj read as text: [(vertices [3, 3] float32, copies, first original index)] of
    every face that occurs more than once, the larger stack first -- 130 and 40 coincident triangles, each
    stack one leaf (binned_sah_builder.hpp:199-232 cannot split equal centroids).  The file is all `v x y z`
    and `f a b c` lines with positive indices."""
    verts, faces = [], []
    with open(DUPLEAF_OBJ) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "v":
                verts.append([float(x) for x in w[1:4]])
            elif w and w[0] == "f":
                faces.append(tuple(int(x) - 1 for x in w[1:4]))
    verts = np.asarray(verts, np.float64).astype(F)
    seen = {}
    for k, face in enumerate(faces):
        seen.setdefault(face, []).append(k)
    stacks = [(verts[list(face)], len(ks), ks[0]) for face, ks in seen.items() if len(ks) > 1]
    stacks.sort(key=lambda s: -s[1])
    assert [s[1] for s in stacks] == [130, 40], [s[1] for s in stacks]
    return stacks


def _model_t(vertices, rays):
    """Triangle::intersect's t of each ray on one triangle, contraction-free float32 (the exact builds')."""
    mesh = types.SimpleNamespace(tri=_tri_rows(vertices[None]))
    return tc.moller_trumbore(mesh, rays, np.zeros(len(rays), np.int64))[0]


@functools.lru_cache(maxsize=None)
def dupleaf_stack_rays():
    """320 rays against the dupleaf scene (floor at z = 1 behind stacks of 130 and 40 coincident triangles),
    fixed seed, the groups interleaved by a fixed permutation so that every wavefront mixes them.  Per stack:
    48 rays along +-z through interior points of the stacked triangle, from in front of it and from behind the
    floor; 48 at a slant from 3 units away on either side, the direction (target - origin) 2^k as rounded
    (k in [-4, 4]); these 96 with windows from tc.WINDOW_TMIN x WINDOW_TMAX.  Per stack 24 rays whose window
    ends or begins exactly at the stack: t0 is this ray's t on the stacked triangle in contraction-free
    float32 (_model_t), the windows [0, t0], [0, nextafter(t0, 0)], [t0, FLT_MAX], [nextafter(t0, inf),
    FLT_MAX], [t0, t0] and [-2, t0], on straight and on slanted rays.  16 rays pass through an interior point
    of both stacks, open windows (170 hits of two t values, with the floor triangle behind them).  64 rays
    are meant to miss: aimed away from the scene, towards a point of z = 1 past the floor's edge (a few of
    these cross a stack on the way), or straight at a stack with tmax = 0."""
    stacks = dupleaf_stacks()
    rng = np.random.default_rng(20261026)

    def interior(v, m):
        a, b = rng.uniform(0.15, 0.4, m), rng.uniform(0.15, 0.4, m)
        v = v.astype(np.float64)
        return v[0] + a[:, None] * (v[1] - v[0]) + b[:, None] * (v[2] - v[0])

    def straight(v, m):
        p = interior(v, m)
        up = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)                 # +z: stack then floor; -z: floor then stack
        o = p.copy()
        o[:, 2] -= up * np.where(up > 0, 2.0, 3.0)
        d = np.zeros((m, 3))
        d[:, 2] = up * np.exp2(rng.integers(-4, 5, m))
        return o, d

    def slanted(v, m):
        p = interior(v, m)
        e = rng.normal(size=(m, 3))
        e[:, 2] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * (0.6 + np.abs(e[:, 2]))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        o = (p + 3.0 * e).astype(F).astype(np.float64)
        return o, (p - o) * np.exp2(rng.integers(-4, 5, m))[:, None]

    def rows(o, d, tmin, tmax):
        r = np.zeros((len(o), 8), F)
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, tmin, tmax
        return r

    parts = []
    for v, _, _ in stacks:
        for make in (straight, slanted):
            o, d = make(v, 48)
            parts.append(rows(o, d, tc.WINDOW_TMIN[rng.integers(0, 4, 48)], tc.WINDOW_TMAX[rng.integers(0, 4, 48)]))
        o, d = straight(v, 12)
        o2, d2 = slanted(v, 12)
        r = rows(np.concatenate([o, o2]), np.concatenate([d, d2]), 0, tc.FLT_MAX)
        t0 = _model_t(v, r)
        assert np.isfinite(t0).all() and (t0 > 0).all()
        k = np.arange(24) % 6
        r[:, 6] = np.select([k == 2, k == 3, k == 4, k == 5], [t0, np.nextafter(t0, F(np.inf)), t0, F(-2)], F(0))
        r[:, 7] = np.select([k == 0, k == 1, k == 4, k == 5], [t0, np.nextafter(t0, F(0)), t0, t0], tc.FLT_MAX)
        parts.append(r)
    pa, pb = interior(stacks[0][0], 16), interior(stacks[1][0], 16)
    flip = (np.arange(16) % 2 == 1)[:, None]
    a, b = np.where(flip, pb, pa), np.where(flip, pa, pb)
    o = (a - 1.5 * (b - a)).astype(F).astype(np.float64)
    parts.append(rows(o, (a - o) * np.exp2(rng.integers(-2, 3, 16))[:, None], 0, tc.FLT_MAX))
    o, d = straight(stacks[0][0], 16)
    away = rows(o, -d, 0, tc.FLT_MAX)                                   # the scene lies behind them
    o = rng.uniform(-1, 1, (32, 3)) * (2.6, 1.9, 1.0) - (0, 0, 2.5)
    target = rng.uniform(-1, 1, (32, 3)) * (2.0, 2.0, 0.0) + (6.0, 0, 1.0) * np.where(np.arange(32) % 2, 1, -1)[:, None]
    target[:, 2] = 1.0
    past = rows(o, target - o, 0, tc.FLT_MAX)                           # cross z = 1 outside the floor, |x| >= 4
    o, d = straight(stacks[1][0], 16)
    parts += [away, past, rows(o, d, 0, 0)]
    rays = np.concatenate(parts)
    assert len(rays) == 320
    rays = np.ascontiguousarray(rays[rng.permutation(len(rays))])
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def soup_rays(name):
    """1,024 rays against a soup of soup_common.RENDERED, fixed seed: origins on the sphere of radius 12
    about 0, each aimed at a point uniform in [-5, 5)^3 (where the finite triangles lie), direction
    (target - origin) 2^k as rounded (k in [-4, 4], the target at t = 2^-k), windows from tc.WINDOW_TMIN x
    WINDOW_TMAX; the last eight rays carry a non-finite float each (tc.DEEP_SPECIALS: the float's index in
    the ray, the value), open windows otherwise."""
    kind, n = SOUP_SETS[name]
    rng = np.random.default_rng([20261027, n, soup_common.KINDS.index(kind)])
    m = SOUP_RAYS
    e = rng.normal(size=(m, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    rays = np.zeros((m, 8), F)
    rays[:, 0:3] = (SOUP_RADIUS * e).astype(F)
    target = rng.uniform(-5, 5, (m, 3))
    rays[:, 3:6] = ((target - rays[:, 0:3]) * np.exp2(rng.integers(-4, 5, m))[:, None]).astype(F)
    rays[:, 6] = tc.WINDOW_TMIN[rng.integers(0, 4, m)]
    rays[:, 7] = tc.WINDOW_TMAX[rng.integers(0, 4, m)]
    for k, (col, value) in enumerate(tc.DEEP_SPECIALS[:SOUP_SPECIALS]):
        row = m - SOUP_SPECIALS + k
        rays[row, 6:8] = (0, tc.FLT_MAX)
        rays[row, col] = value
    rays.setflags(write=False)
    return rays


def new_set_rays(name):
    """The generator of a new set's rays (the fixture stores its output)."""
    return dupleaf_stack_rays() if name == DUPLEAF else soup_rays(name)


def rays_sha256(rays):
    return hashlib.sha256(np.ascontiguousarray(rays, F).tobytes()).hexdigest()


def sort_and_truncate(counts, rec):
    """The stored form of the walk-order records `rec` (structured, ray after ray, counts[k] each): per ray a
    stable sort by the product's key -- t by float <, equal t (-0 == +0) by original triangle index, the sort
    of model_ray -- then the first min(count, 32).  Returns the kept records, ray after ray."""
    ray = np.repeat(np.arange(len(counts)), counts.astype(np.int64))
    t = rec["t"].view(F)
    assert not np.isnan(t).any()
    order = np.lexsort((rec["prim"], t, ray))                         # stable; float keys compare -0 == +0
    start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])[:-1]
    rank = np.arange(len(rec)) - np.repeat(start, counts.astype(np.int64))
    return rec[order][rank < MAX_HITS]                                # ray is the slowest key: rank stays valid


@functools.lru_cache(maxsize=None)
def load_all_fixture(name):
    """tests/golden/rays_all/<name>.npz (or <name>.<variant>.npz where one file would pass the size limit):
    {"rays": float32 [n, 8], variant: {"count", "steps", "tests": uint32 [n], "rows": [n, 32] HIT_DTYPE, the
    first min(count, 32) records then misses {-1, 0, 0, 0}}}; read-only, loaded once.  The rays are the stored
    ones (new sets) or those of tests/golden/rays/<name>.npz, whose sha256 the file holds -- verified."""
    one = os.path.join(ALL_DIR, name + ".npz")
    files = [np.load(one)] if os.path.exists(one) else [np.load(os.path.join(ALL_DIR, "%s.%s.npz" % (name, v))) for v in tc.RAY_VARIANTS]
    z = {k: f[k] for f in files for k in f.files}
    rays = z["rays"] if "rays" in z else tc.load_ray_fixture(name)["rays"]
    assert rays.dtype == F and rays.shape[1] == 8
    assert bytes(z["rays_sha256"]).decode() == rays_sha256(rays), name
    out = {"rays": rays}
    n = len(rays)
    for v in tc.RAY_VARIANTS:
        count = z[v + "_count"]
        kept = np.minimum(count, MAX_HITS).astype(np.int64)
        assert count.shape == (n,) and len(z[v + "_prim"]) == kept.sum()
        rows = np.zeros((n, MAX_HITS), HIT_DTYPE)
        rows["prim"] = -1
        real = np.arange(MAX_HITS)[None, :] < kept[:, None]
        rows["prim"][real] = z[v + "_prim"]
        for k in ("t", "u", "v"):
            rows[k][real] = z[v + "_" + k].view(F)
        out[v] = {"count": count, "steps": z[v + "_steps"], "tests": z[v + "_tests"], "rows": rows}
    for a in [out["rays"]] + [a for v in tc.RAY_VARIANTS for a in out[v].values()]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def all_set_scene(name, arith=0):
    """(mesh, bvh) of any set of ALL_SETS, prepared in the given arithmetic (host builder)."""
    pkg = import_package()
    if name in SOUP_SETS:
        mesh = soup_common.mesh_of(pkg, *SOUP_SETS[name])
        return mesh, pkg.build_bvh(mesh, arith=arith)
    if name == DUPLEAF:
        return tc.fixture("dupleaf", arith)[1:3]
    return tc.ray_set_scene(name, arith)


def scene_key(name):
    """What names a set's scene (several sets share one)."""
    if name in NEW_SETS:
        return name
    return "proc300" if name == "proc300_window" else tc.ray_set_config(name)["obj"]


def check_against_all_fixture(pkg, trace_all, name, variant, stats, prefixes=(1, 5)):
    """trace_all on the set's scene prepared for `variant` must return what the reference's traverser gave the
    collecting intersector, bit for bit: at max_hits = 32 the counts and the rows (misses {-1, 0, 0, 0}); at
    max_hits 1 and 5 the prefix of the stored row; the count-only call the counts; stats["hits"] the number of
    rays with a hit.  stats (the CPU path, GPU stats scenes): as in tc.check_against_ray_fixture the rays
    none of whose floats is NaN go in one call and the others in a call of their own, and each call's
    node_pairs / tri_tests are the sums of the reference's traversal_steps / intersections over its rays.
    Otherwise one call in stored order."""
    fx = load_all_fixture(name)
    ref = fx[variant]
    mode, _ = tc.variant_mode(pkg, variant)
    idx = np.arange(len(fx["rays"]))
    parts = [idx]
    if stats:
        nan = np.isnan(fx["rays"]).any(axis=1)
        parts = [idx[~nan]] + ([idx[nan]] if nan.any() else [])
    for k, part in enumerate(parts):
        rays = np.ascontiguousarray(fx["rays"][part])
        exp_c, exp_r = ref["count"][part], np.ascontiguousarray(ref["rows"][part])
        n_hit = int((exp_c >= 1).sum())
        for K in (MAX_HITS,) + tuple(prefixes) + (0,):
            where = (name, variant, "stats" if stats else "production", "part %d" % k, "max_hits %d" % K)
            c, r, st = trace_all(rays, K, mode, K > 0)
            assert np.array_equal(c, exp_c), (where, "counts: first differing rays", part[np.flatnonzero(c != exp_c)[:8]])
            if K:
                e = np.ascontiguousarray(exp_r[:, :K])
                bad = np.flatnonzero((r.view(np.uint32) != e.view(np.uint32)).reshape(len(part), -1).any(axis=1))
                assert rows_equal(r, e), (where, "rows: first differing rays", part[bad[:8]])
            else:
                assert r is None, where
            assert st["rays"] == len(part) and st["hits"] == n_hit, where
            if stats:
                assert st["node_pairs"] == int(ref["steps"][part].sum(dtype=np.uint64)), where
                assert st["tri_tests"] == int(ref["tests"][part].sum(dtype=np.uint64)), where


def check_all_fixture_floors():
    """What keeps the fixture comparisons from passing vacuously, on the stored reference answers alone."""
    fx = load_all_fixture(DUPLEAF)
    sizes = [s[1] for s in dupleaf_stacks()]
    for v in tc.RAY_VARIANTS:
        c, rows = fx[v]["count"], fx[v]["rows"]
        assert (c > MAX_HITS).sum() >= 20 and (c >= sizes[0]).any() and ((c >= sizes[1]) & (c < sizes[0])).any() and (c == 0).any(), v
        full = c > MAX_HITS                                           # a full list of records equal in t: order and
        same_t = (rows["t"][full] == rows["t"][full][:, :1]).all(axis=1)   # eviction decided by original index alone
        assert same_t.sum() >= 20, v
        assert (np.diff(rows["prim"][full][same_t].astype(np.int64), axis=1) > 0).all(), v
    for name in SOUP_SETS:
        fx = load_all_fixture(name)
        assert np.isnan(fx["rays"]).any() and np.isinf(fx["rays"][:, :6]).any(), name
        for v in tc.RAY_VARIANTS:
            c = fx[v]["count"]
            if c.any():
                assert (c > 1).any() and (c == 0).any(), (name, v)
    differ = 0
    for name in ALL_SETS:                                             # the variants differ in substance
        fx = load_all_fixture(name)
        for a, b in (("exact_fast", "exact_robust"), ("exact_fast", "ref_fast"), ("ref_fast", "ref_robust")):
            differ += int((fx[a]["count"] != fx[b]["count"]).sum())
    assert differ > 0
