"""Shared pieces of the all-hits ray-query tests (test_allhits_cpu.py, test_gpu_allhits.py).

The hit set of a ray is what the reference's SingleRayTraverser::traverse presents to an intersector
that never lowers ray.tmax: the BVH2 walk of single_ray_traverser.hpp:68-126 with every box test and
every triangle test against the ray's original [tmin, tmax].  model() below is that walk in Python over
the reference-layout nodes (bvh.nodes, bvh.prim) -- the FastNodeIntersector in contraction-free float32,
its fma rounded once from the exact value -- and the checks every path must pass, each taking a
`trace_all(rays, max_hits, mode, hits) -> (counts, rows | None, stats)` callable."""
import functools
from fractions import Fraction

import numpy as np

import trace_common as tc
from conftest import import_package
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
