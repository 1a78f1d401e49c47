"""Shared pieces of the all-hits and complete-hit-list tests on double scenes (test_allhits_cpu_f64.py,
test_gpu_allhits_f64.py).

The reference harness has no all-hits mode in its double builds, so nothing here is reference-made.  The
double queries are pinned by what exists: model_rays() below -- the fixed-window walk of
single_ray_traverser.hpp:68-126 in Python float64 over the reference-layout nodes, allhits_common.model_ray's
sibling: octant-picked bounds, the robust_max / robust_min nesting, safe_inverse with DBL_EPSILON, the box
test's fma rounded once from the exact value; Moller-Trumbore contraction-free (trace64_common's) or with the
fmas of dev64::dotA / dotB / crossG (oracle/contraction_sites.txt) -- the reference's stored closest answers
of tests/golden/rays64/, a brute force over all triangles, and the properties of sorted lists.  Every path is
a `trace_all(rays, max_hits, mode, hits) -> (counts, rows | None, stats)` or a `trace_lists(rays, mode) ->
(offsets, hits, stats)` callable."""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

import allhits_common as ac
import soup_common
import trace64_common as t64
from conftest import import_package
from refit_common import node_fields

D = np.float64
MAX_HITS = 32
EPS = float(np.finfo(np.float64).eps)
MODEL_SETS = {"tri1_tiny64": None, "quad_tiny64": None, "lattice_ties64": None, "dragon_adversarial64": 512}   # set -> first n rays
VARIANTS = t64.RAY_VARIANTS64                                         # exact_fast (mode 0), ref_fast (MODE_FMA, arith 1)
PREFIX_K = (1, 2, 5, 8)
DUPLEAF64 = "dupleaf_stack64"
NANBOX64 = "nan_leaf_soup64"
BRUTE_SHARE = 0.01                                                    # rays the brute-force comparison may exclude
_SAFE_LO, _SAFE_HI = 2.0 ** -900, 2.0 ** 900                          # where the error-free transforms below are exact


# ---------------------------------------------------------------- float64 fma, rounded once

def _fma_exact(a, b, c):
    """The exact rational a b + c of three finite doubles, rounded once."""
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.copysign(math.inf, a * b if a * b != 0 else c)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                               # 2^27 + 1 (Veltkamp)
    h = c - (c - a)
    return h, a - h


def fma(a, b, c):
    """fma(a, b, c) in float64, the exact a b + c rounded once.  Finite operands of moderate size go through
    Boldo and Melquiond's emulation (an exact product, two exact sums, the two low parts added with rounding
    to odd); anything else through the exact rational (trace64_common.fma) or, with a non-finite operand,
    the plain expression, whose inf / NaN is the fma's."""
    a, b, c = float(a), float(b), float(c)
    p = a * b
    if not (math.isfinite(p) and math.isfinite(c) and math.isfinite(a) and math.isfinite(b)):
        if math.isfinite(a) and math.isfinite(b) and math.isfinite(c):
            return _fma_exact(a, b, c)                                # the product alone overflows
        if math.isfinite(a) and math.isfinite(b) and math.isinf(c):
            return c                                                  # the exact product is finite
        with np.errstate(all="ignore"):
            return float(D(a) * D(b) + D(c))
    if a == 0.0 or b == 0.0:
        return p + c                                                  # exact, and the sign of a zero sum is IEEE's
    if p == 0.0 or not (_SAFE_LO < abs(p) < _SAFE_HI and abs(a) < _SAFE_HI and abs(b) < _SAFE_HI and
                        (c == 0.0 or _SAFE_LO < abs(c) < _SAFE_HI)):
        return _fma_exact(a, b, c)
    ah, al = _split(a)
    bh, bl = _split(b)
    pl = ((ah * bh - p) + ah * bl + al * bh) + al * bl                # p + pl = a b exactly
    uh, ul = _two_sum(c, pl)
    th, tl = _two_sum(p, uh)
    v, e = _two_sum(tl, ul)
    if e != 0.0 and not struct.unpack("<Q", struct.pack("<d", v))[0] & 1:
        v = math.nextafter(v, math.inf if e > 0 else -math.inf)       # round to odd
    return th + v


def fma_np(a, b, c):
    """fma() over arrays (broadcast), element by element the same value."""
    a, b, c = np.broadcast_arrays(np.asarray(a, D), np.asarray(b, D), np.asarray(c, D))
    with np.errstate(all="ignore"):
        p = a * b
        fin = np.isfinite(p) & np.isfinite(c) & np.isfinite(a) & np.isfinite(b)
        safe = fin & (p != 0) & (np.abs(p) > _SAFE_LO) & (np.abs(p) < _SAFE_HI) & (np.abs(a) < _SAFE_HI) & (np.abs(b) < _SAFE_HI) & \
            ((c == 0) | ((np.abs(c) > _SAFE_LO) & (np.abs(c) < _SAFE_HI)))
        ca, cb = 134217729.0 * a, 134217729.0 * b
        ah, bh = ca - (ca - a), cb - (cb - b)
        al, bl = a - ah, b - bh
        pl = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        uh, ul = _two_sum(c, pl)
        th, tl = _two_sum(p, uh)
        v, e = _two_sum(tl, ul)
        even = (np.ascontiguousarray(v).view(np.uint64) & np.uint64(1)) == 0
        v = np.where((e != 0) & even, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
        zero = (a == 0) | (b == 0)                                   # an exact +-0 product: p + c is exact, zero signs IEEE's
        out = np.where(fin & ~zero, th + v, np.where(np.isfinite(a) & np.isfinite(b) & np.isinf(c), c, p + c))
    slow = ~safe & ~zero & np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    if slow.any():
        out, fa, fb, fc = out.reshape(-1), a.reshape(-1), b.reshape(-1), c.reshape(-1)
        for k in np.flatnonzero(slow):
            out[k] = _fma_exact(float(fa[k]), float(fb[k]), float(fc[k]))
        out = out.reshape(a.shape)
    return out


# ---------------------------------------------------------------- Triangle<double>::intersect

def moller_trumbore_fma(tri, rays):
    """triangle.hpp:95-115 in float64 with the reference CMake build's contraction, the sites of
    oracle/contraction_sites.txt as dev64::tri_test<true> carries them: cross a_j b_k - a_k b_j as
    fma(a_j, b_k, -(a_k b_j)); dot "A" fma(a2, b2, fma(a0, b0, a1 b1)) for n.d, r.e2 and n.c; dot "B"
    fma(a2, b2, fma(a1, b1, a0 b0)) for v = r.e1.  (t, u, v) of rays [m, 8] on triangles [m, 12]."""
    p0, e1, e2, n = tri[..., 0:3], tri[..., 3:6], tri[..., 6:9], tri[..., 9:12]
    o, d = rays[..., 0:3], rays[..., 3:6]
    dot_a = lambda a, b: fma_np(a[..., 2], b[..., 2], fma_np(a[..., 0], b[..., 0], a[..., 1] * b[..., 1]))   # noqa: E731
    dot_b = lambda a, b: fma_np(a[..., 2], b[..., 2], fma_np(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))   # noqa: E731
    with np.errstate(all="ignore"):
        c = p0 - o
        r = np.stack([fma_np(d[..., 1], c[..., 2], -(d[..., 2] * c[..., 1])), fma_np(d[..., 2], c[..., 0], -(d[..., 0] * c[..., 2])),
                      fma_np(d[..., 0], c[..., 1], -(d[..., 1] * c[..., 0]))], axis=-1)
        inv_det = D(1) / dot_a(n, d)
        return dot_a(n, c) * inv_det, dot_a(r, e2) * inv_det, dot_b(r, e1) * inv_det


def accepted(tri, rays, contracted=False):
    """(accepted mask, t, u, v) of Triangle<double>::intersect, ray k on triangle row k, in the ray's window."""
    t, u, v = moller_trumbore_fma(tri, rays) if contracted else t64.moller_trumbore(tri, rays)
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (v >= 0) & (D(1) - u - v >= 0) & (t >= rays[..., 6]) & (t <= rays[..., 7]), t, u, v


# ---------------------------------------------------------------- the model

def walk(bounds, count, first, ray):
    """The leaves the fixed-window walk reaches (node indices, in walk order) and its steps: the
    FastNodeIntersector of node_intersectors.hpp:35-47,83-103 in float64."""
    if count[0]:
        return [0], 0
    tmin, tmax = float(ray[6]), float(ray[7])
    with np.errstate(all="ignore"):
        d = ray[3:6]
        inv = D(1) / np.where(np.abs(d) < EPS, np.copysign(EPS, d), d)                       # safe_inverse, vector.hpp:69-74
        so = (-ray[0:3]) * inv
    octant = [int(x) for x in np.signbit(d)]
    inv, so = [float(x) for x in inv], [float(x) for x in so]
    gt = lambda p, q: p if p > q else q                               # noqa: E731  robust_max: the right operand unless p > q
    lt = lambda p, q: p if p < q else q                               # noqa: E731  robust_min

    def box(k):
        b = bounds[k]
        e = [fma(b[2 * a + octant[a]], inv[a], so[a]) for a in range(3)]
        x = [fma(b[2 * a + 1 - octant[a]], inv[a], so[a]) for a in range(3)]
        return gt(e[0], gt(e[1], gt(e[2], tmin))) <= lt(x[0], lt(x[1], lt(x[2], tmax)))

    leaves, steps, stack, left = [], 0, [], first[0]
    while True:
        steps += 1
        go = []
        for k in (left, left + 1):
            if box(k):
                (leaves if count[k] else go).append(k)
        if len(go) == 2:
            stack.append(first[go[1]])
        if go:
            left = first[go[0]]
        elif stack:
            left = stack.pop()
        else:
            break
    return leaves, steps


def model_rays(mesh, bvh, rays, contracted=False):
    """The model's complete answer for `rays`: {"count" u32 [n], "offsets" u64 [n + 1], "hits" HIT64_DTYPE
    [total] in the key order (t ascending by double <, equal t -- -0 == +0 -- by original triangle index),
    "steps", "tests" u64 [n]}.  The walks run ray by ray; the triangle tests of all reached leaves in one
    numpy pass."""
    pkg = import_package()
    bounds, count, first = node_fields(bvh.nodes)
    bounds = [[float(x) for x in row] for row in bounds]
    count, first = [int(x) for x in count], [int(x) for x in first]
    prim = np.asarray(bvh.prim, np.int64)
    n = len(rays)
    steps, tests = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    pr, pp = [], []
    for k in range(n):
        leaves, steps[k] = walk(bounds, count, first, rays[k])
        for node in leaves:
            p = prim[first[node]:first[node] + count[node]]
            tests[k] += len(p)
            pr.append(np.full(len(p), k, np.int64))
            pp.append(p)
    pr = np.concatenate(pr) if pr else np.zeros(0, np.int64)
    pp = np.concatenate(pp) if pp else np.zeros(0, np.int64)
    ok, t, u, v = accepted(mesh.tri[pp], rays[pr], contracted)
    pr, pp, t, u, v = pr[ok], pp[ok], t[ok], u[ok], v[ok]
    order = np.lexsort((pp, t, pr))                                   # float keys compare -0 == +0
    hits = np.zeros(len(order), pkg.HIT64_DTYPE)
    hits["prim"], hits["t"], hits["u"], hits["v"] = pp[order], t[order], u[order], v[order]
    cnt = np.bincount(pr, minlength=n).astype(np.uint32)
    out = {"count": cnt, "offsets": offsets_of(cnt), "hits": hits, "steps": steps, "tests": tests}
    for a in out.values():
        a.setflags(write=False)
    return out


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)


def rows_of(m, K=MAX_HITS):
    """A model answer's [n, K] rows: the first min(count, K) records of each list, then misses."""
    pkg = import_package()
    n = len(m["count"])
    rows = np.zeros((n, K), pkg.HIT64_DTYPE)
    rows["prim"] = -1
    kept = np.minimum(m["count"], K).astype(np.int64)
    real = np.arange(K)[None, :] < kept[:, None]
    src = (m["offsets"][:-1].astype(np.int64)[:, None] + np.arange(K)[None, :])[real]
    rows[real] = m["hits"][src]
    return rows


def contracted_of(variant):
    return variant == "ref_fast"


def build_of(variant):
    return "ref" if variant == "ref_fast" else "exact"


@functools.lru_cache(maxsize=None)
def dupleaf64(build="exact"):
    """(mesh, bvh) of tests/golden/dupleaf.obj as a double scene: leaves of 130 and 40 coincident triangles."""
    pkg = import_package()
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["dupleaf"], f64=True, arith=1 if build == "ref" else 0)
    return mesh, bvh


@functools.lru_cache(maxsize=None)
def nanbox64():
    """(mesh, bvh, rays): soup_common's float recipe widened to double -- soup("nan_p0", 300), whose
    poisoned triangles have a NaN p0 component -- plus eight triangles NaN on x in all three vertices and
    otherwise packed in one small cell far from the rest, so that the builder gives them a leaf (or leaves) of
    their own, whose box stays inverted on x.  1,024 rays from the sphere of radius 12 at targets in the
    soup's cube and in that cell."""
    pkg = import_package()
    tri, _ = soup_common.soup("nan_p0", 300)
    rng = np.random.default_rng(20261028)
    p = (np.array([40.0, 40.0, 40.0]) + rng.uniform(-0.5, 0.5, (8, 3, 3)))
    p[:, :, 0] = np.nan
    p0, e1, e2 = p[:, 0], p[:, 0] - p[:, 1], p[:, 2] - p[:, 0]
    with np.errstate(invalid="ignore"):
        nrm = np.cross(e1, e2)
    with np.errstate(invalid="ignore"):                              # (signalling NaNs of the float recipe)
        tri = np.concatenate([tri.astype(D), np.concatenate([p0, e1, e2, nrm], axis=1)])
    mesh = pkg.Mesh(tri, np.concatenate([soup_common.normals(tri[:300].astype(np.float32)).astype(D), np.zeros((8, 9))]))
    bvh = pkg.build_bvh(mesh)
    m = 1024
    e = rng.normal(size=(m, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    rays = np.zeros((m, 8), D)
    rays[:, 0:3] = 12.0 * e
    target = np.where((np.arange(m) % 4 == 0)[:, None], 40.0 + rng.uniform(-0.5, 0.5, (m, 3)), rng.uniform(-5, 5, (m, 3)))
    rays[:, 3:6] = (target - rays[:, 0:3]) * np.exp2(rng.integers(-4, 5, m))[:, None]
    rays[:, 6] = t64.WINDOW_TMIN[rng.integers(0, 4, m)]
    rays[:, 7] = t64.WINDOW_TMAX[rng.integers(0, 4, m)]
    rays.setflags(write=False)
    return mesh, bvh, rays


def inverted_leaves(bvh):
    """Leaves of a double BVH whose box is inverted (lo > hi) on some axis."""
    bounds, count, _ = node_fields(bvh.nodes)
    return np.flatnonzero((count > 0) & (bounds[:, 0::2] > bounds[:, 1::2]).any(axis=1))


def set_scene(name, build="exact"):
    """(mesh, bvh) of a model set, the dupleaf scene or the NaN-leaf soup."""
    if name == DUPLEAF64:
        return dupleaf64(build)
    if name == NANBOX64:
        return nanbox64()[:2]
    if name in t64.BRUTE_SCENES:
        return t64.brute_scene(name)
    return t64.ray_set_scene(name, build)


def set_rays(name):
    if name == DUPLEAF64:
        return np.ascontiguousarray(ac.dupleaf_stack_rays().astype(D))
    if name == NANBOX64:
        return nanbox64()[2]
    if name in t64.BRUTE_SCENES:
        return t64.brute_rays(name)
    return np.ascontiguousarray(t64.load_ray_fixture64(name)["rays"][:MODEL_SETS.get(name)])


@functools.lru_cache(maxsize=None)
def model(name, variant="exact_fast"):
    """model_rays of a set's (first MODEL_SETS[name]) rays on its scene prepared for `variant`, computed once."""
    mesh, bvh = set_scene(name, build_of(variant))
    return model_rays(mesh, bvh, set_rays(name), contracted_of(variant))


# ---------------------------------------------------------------- brute force

@functools.lru_cache(maxsize=None)
def brute_accepted(name):
    """[n rays, n triangles] bool: Triangle<double>::intersect accepts, contraction-free, every pair (small
    scenes only).  NOT the definition of the hit set: the walk tests a triangle only behind its boxes."""
    mesh, _ = set_scene(name)
    rays = set_rays(name)
    out = np.zeros((len(rays), len(mesh)), bool)
    tri = mesh.tri[None, :, :]
    for k0 in range(0, len(rays), 256):
        r = rays[k0:k0 + 256]
        out[k0:k0 + 256] = accepted(tri, r[:, None, :])[0]
    out.setflags(write=False)
    return out


def model_sets(name):
    """[n rays, n triangles] bool of the model's exact_fast hit sets."""
    m = model(name)
    out = np.zeros((len(m["count"]), len(set_scene(name)[0])), bool)
    out[np.repeat(np.arange(len(m["count"])), m["count"].astype(np.int64)), m["hits"]["prim"]] = True
    return out


def brute_keep(name):
    """The rays the brute-force comparison keeps: those whose model set is the brute force's.  The cap, from
    the model and numpy alone: at most 1 % excluded, at least 10 % with a hit and 10 % without among the
    rest."""
    brute, walked = brute_accepted(name), model_sets(name)
    assert not (walked & ~brute).any(), name                          # the walk's set is a subset
    keep = (brute == walked).all(axis=1)
    n = len(keep)
    assert n == t64.BRUTE_N and (~keep).sum() <= BRUTE_SHARE * n, (name, int((~keep).sum()))
    hit = brute.any(axis=1)
    assert (hit & keep).sum() >= 0.10 * n and (~hit & keep).sum() >= 0.10 * n, (name, int((hit & keep).sum()))
    return keep


def check_against_brute_force(trace_all, name):
    """Per kept ray: count is the number of triangles the brute force accepts, and where count <= 32 the
    listed prims are that set."""
    keep = brute_keep(name)
    brute = brute_accepted(name)
    counts, rows, _ = trace_all(set_rays(name), MAX_HITS, 0, True)
    assert np.array_equal(counts[keep], brute.sum(axis=1)[keep]), (name, np.flatnonzero(keep & (counts != brute.sum(axis=1)))[:8])
    for k in np.flatnonzero(keep & (counts <= MAX_HITS)):
        assert set(rows["prim"][k, :counts[k]].tolist()) == set(np.flatnonzero(brute[k]).tolist()), (name, k)


# ---------------------------------------------------------------- the checks

def words(a):
    """Records as 4 x uint64 words each (prim and pad share the first)."""
    return np.ascontiguousarray(a).view(np.uint64).reshape(a.shape + (4,))


def rows_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_bad(a, b):
    """The first rays (rows) or records (lists) that differ, for messages."""
    if a.shape != b.shape:
        return ("shapes", a.shape, b.shape)
    return np.flatnonzero((words(a) != words(b)).reshape(len(a), -1).any(axis=1))[:8].tolist()


def nan_parts(rays, stats):
    """One call, or (stats: the CPU path, GPU stats scenes) the rays without a NaN in one call and the others
    in a call of their own, as allhits_common.check_against_all_fixture."""
    idx = np.arange(len(rays))
    if not stats:
        return [idx]
    nan = np.isnan(rays).any(axis=1)
    return [idx[~nan]] + ([idx[nan]] if nan.any() else [])


def check_against_model(pkg, trace_all, name, variant, stats, prefixes=(1, 5)):
    """trace_all on the set's scene prepared for `variant` returns the model's answer bit for bit: counts and
    rows at max_hits = 32, prefixes at 1 and 5, the count-only counts, stats rays / hits, and with `stats`
    node_pairs / tri_tests."""
    m, rays_all = model(name, variant), set_rays(name)
    rows_all = rows_of(m)
    mode = t64.variant_mode(pkg, variant)[0]
    for k, part in enumerate(nan_parts(rays_all, stats)):
        rays = np.ascontiguousarray(rays_all[part])
        exp_c, exp_r = m["count"][part], np.ascontiguousarray(rows_all[part])
        for K in (MAX_HITS,) + tuple(prefixes) + (0,):
            where = (name, variant, "stats" if stats else "production", "part %d" % k, "max_hits %d" % K)
            c, r, st = trace_all(rays, K, mode, K > 0)
            assert np.array_equal(c, exp_c), (where, "counts: first differing rays", part[np.flatnonzero(c != exp_c)[:8]])
            if K:
                assert r.dtype == pkg.HIT64_DTYPE, where
                e = np.ascontiguousarray(exp_r[:, :K])
                assert rows_equal(r, e), (where, "rows: first differing rays", part[first_bad(r, e)])
            else:
                assert r is None, where
            assert st["rays"] == len(part) and st["hits"] == int((exp_c >= 1).sum()), where
            if stats:
                assert st["node_pairs"] == int(m["steps"][part].sum()), (where, st["node_pairs"], int(m["steps"][part].sum()))
                assert st["tri_tests"] == int(m["tests"][part].sum()), (where, st["tri_tests"], int(m["tests"][part].sum()))


def check_lists_against_model(pkg, trace_lists, name, variant, stats):
    """trace_lists returns the model's complete lists bit for bit, offsets = [0] + cumsum(counts)."""
    m, rays_all = model(name, variant), set_rays(name)
    mode = t64.variant_mode(pkg, variant)[0]
    for k, part in enumerate(nan_parts(rays_all, stats)):
        where = (name, variant, "stats" if stats else "production", "part %d" % k)
        cnt = m["count"][part]
        exp = np.concatenate([m["hits"][int(m["offsets"][r]):int(m["offsets"][r + 1])] for r in part]) if len(part) else m["hits"][:0]
        off, hits, st = trace_lists(np.ascontiguousarray(rays_all[part]), mode)
        assert off.dtype == np.uint64 and np.array_equal(off, offsets_of(cnt)), (where, "offsets")
        assert hits.dtype == pkg.HIT64_DTYPE and rows_equal(hits, exp), (where, "first differing records", first_bad(hits, exp))
        assert st["rays"] == len(part) and st["hits"] == int((cnt >= 1).sum()), where
        if stats:
            assert st["node_pairs"] == int(m["steps"][part].sum()) and st["tri_tests"] == int(m["tests"][part].sum()), where


def check_against_reference_answers(pkg, trace_all, name, variant):
    """allhits_common.check_against_reference_answers against tests/golden/rays64/: count >= 1 exactly where
    the reference's occluded is 1; the reference's closest record is one of the listed records, bit for bit,
    where count <= 32; the first listed t is <= the reference's t; stats.hits is the reference's occluded
    count."""
    fx = t64.load_ray_fixture64(name)
    ref = fx[variant]
    mode = t64.variant_mode(pkg, variant)[0]
    counts, rows, st = trace_all(fx["rays"], MAX_HITS, mode, True)
    occ = ref["occluded"].astype(bool)
    assert np.array_equal(counts >= 1, occ), (name, variant, np.flatnonzero((counts >= 1) != occ)[:8])
    assert st["rays"] == len(fx["rays"]) and st["hits"] == int(occ.sum()), (name, variant)
    exp = t64.reference_hits(pkg, ref)
    hit = exp["prim"] >= 0
    assert np.array_equal(hit, occ)
    listed = hit & (counts <= MAX_HITS)
    same = (words(rows) == words(exp)[:, None, :]).all(axis=2).any(axis=1)
    assert same[listed].all(), (name, variant, np.flatnonzero(listed & ~same)[:8])
    assert (rows["t"][hit, 0] <= exp["t"][hit]).all(), (name, variant)
    return counts, rows


def check_rows(rays, counts, rows, K):
    """A [n, K] answer is well formed: rows sorted by the key, prims distinct, every t inside the ray's
    window, min(count, K) records then misses that are all-zero after prim = -1; pad 0 everywhere."""
    n = len(rays)
    assert counts.shape == (n,) and counts.dtype == np.uint32 and rows.shape == (n, K)
    assert not rows["pad"].any()
    kept = np.minimum(counts, K).astype(np.int64)
    real = np.arange(K)[None, :] < kept[:, None]
    assert np.array_equal(rows["prim"] >= 0, real)
    miss = rows[~real]
    assert (miss["prim"] == -1).all()
    for f in ("t", "u", "v"):
        assert not np.ascontiguousarray(miss[f]).view(np.uint64).any(), f
    t, p = rows["t"], rows["prim"]
    assert not np.isnan(t[real]).any()
    assert ((t >= rays[:, 6:7]) & (t <= rays[:, 7:8]))[real].all()
    pair = real[:, 1:]
    a, b, pa, pb = t[:, :-1], t[:, 1:], p[:, :-1], p[:, 1:]
    assert ((a < b) | ((a == b) & (pa < pb)))[pair].all()             # strictly increasing key: prims distinct too
    for k in np.flatnonzero(kept > 1):
        assert len(set(p[k, :kept[k]].tolist())) == kept[k]


def check_list_properties(trace_all, rays, mode):
    """allhits_common.check_list_properties for HIT64_DTYPE rows.  Returns (counts, rows at 32)."""
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


def check_lists(rays, offsets, hits):
    """hitlists_common.check_lists for HIT64_DTYPE records."""
    n = len(rays)
    assert offsets.shape == (n + 1,) and offsets.dtype == np.uint64 and offsets[0] == 0 and offsets[n] == len(hits)
    counts = np.diff(offsets.astype(np.int64))
    assert (counts >= 0).all() and not hits["pad"].any()
    ray = np.repeat(np.arange(n), counts)
    t, p = hits["t"], hits["prim"]
    assert (p >= 0).all() and not np.isnan(t).any()
    assert ((t >= rays[ray, 6]) & (t <= rays[ray, 7])).all()
    same = ray[1:] == ray[:-1]
    a, b, pa, pb = t[:-1], t[1:], p[:-1], p[1:]
    assert ((a < b) | ((a == b) & (pa < pb)))[same].all()


def check_lists_against_trace_all(trace_lists, trace_all, rays, mode):
    """Against the capped query: counts equal; each list's first min(count, 32) records are the max_hits = 32
    row; check_lists; a permutation of the rays permutes the lists.  Returns (offsets, hits)."""
    rays = np.ascontiguousarray(rays)
    off, hits, st = trace_lists(rays, mode)
    counts, rows, st32 = trace_all(rays, MAX_HITS, mode, True)
    check_lists(rays, off, hits)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts.astype(np.int64))
    assert (st["rays"], st["hits"]) == (st32["rays"], st32["hits"]) == (len(rays), int((counts >= 1).sum()))
    kept = np.minimum(counts, MAX_HITS).astype(np.int64)
    real = np.arange(MAX_HITS)[None, :] < kept[:, None]
    src = (off[:-1].astype(np.int64)[:, None] + np.arange(MAX_HITS)[None, :])[real]
    assert rows_equal(np.ascontiguousarray(hits[src]), np.ascontiguousarray(rows[real]))
    perm = np.random.default_rng(20261029).permutation(len(rays))
    o2, h2, _ = trace_lists(rays[perm], mode)
    assert np.array_equal(np.diff(o2.astype(np.int64)), counts[perm].astype(np.int64))
    seg = [hits[int(off[r]):int(off[r + 1])] for r in perm]
    assert rows_equal(h2, np.concatenate(seg) if len(hits) else hits)
    return off, hits


def check_dupleaf_floors(variant):
    """From the model alone: at least 20 rays with count > 32 whose 32 records share one t and ascend in prim;
    segments of at least 130 and of 40 .. 129 records; empty ones."""
    m = model(DUPLEAF64, variant)
    c, rows = m["count"], rows_of(m)
    full = c > MAX_HITS
    same_t = (rows["t"][full] == rows["t"][full][:, :1]).all(axis=1)
    assert same_t.sum() >= 20, (variant, int(same_t.sum()))
    assert (np.diff(rows["prim"][full][same_t].astype(np.int64), axis=1) > 0).all(), variant
    assert (c >= 130).any() and ((c >= 40) & (c < 130)).any() and (c == 0).any(), variant
