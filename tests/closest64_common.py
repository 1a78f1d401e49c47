"""What the double closest-point tests share (test_closest_cpu_f64.py, test_gpu_closest_f64.py): the float64
model that is the oracle of both paths, the point sets, the scenes.

The contract (include/ceres_render.h "closest-point queries on double-precision scenes") is the float one with
float replaced by double: the answer is the minimum over ALL triangles of one float64 formula, ties to the
smallest original index, whatever the tree.  model64_exact is that brute force over closest_common.pair_d2 in
float64; numpy's float64 + - * / are the IEEE operations the library compiles, so the comparison is byte for
byte.  (closest_common.model32 / model64 cast the mesh to float32 and cannot serve here.)"""
import functools

import numpy as np

import closest_common as cc
import deep_common as dc

D = np.float64
NEAR64_DTYPE = np.dtype([("prim", np.int32), ("pad", np.int32), ("d2", np.float64), ("u", np.float64), ("v", np.float64)])
SCENES = cc.SCENES
ORDER = cc.ORDER
PER_SET = cc.PER_SET
FAR = np.asarray([2.0 ** 27, -2.0 ** 26, 2.0 ** 25])                   # bunny_far's translation


def model64_exact(tri, points):
    """near32 records [n] of points [n, 4] float64 over tri [m, 12] float64 (original order): the smallest
    d2 <= r2max, the first index among equals; misses {-1, 0, 0, 0, 0}."""
    tri = np.asarray(tri, D).reshape(-1, 12)
    points = np.asarray(points, D).reshape(-1, 4)
    out = np.zeros(len(points), NEAR64_DTYPE)
    out["prim"] = -1
    step = max(1, cc.CHUNK // len(tri))
    for s in range(0, len(points), step):
        pts = points[s:s + step]
        d2, v, w = cc.pair_d2(tri, pts, D, clamp=True)
        with np.errstate(all="ignore"):
            ok = d2 <= pts[:, 3, None]                                # NaN d2, NaN or negative r2max: never
        key = np.where(ok, d2, np.inf)
        cand = ok & (key == key.min(axis=1, keepdims=True))
        best = cand.argmax(axis=1)                                    # the first index of the minimum
        rows = np.arange(len(pts))
        found = cand[rows, best]
        o = out[s:s + step]
        o["prim"] = np.where(found, best, -1)
        o["d2"] = np.where(found, d2[rows, best], 0.0)
        o["u"] = np.where(found, v[rows, best], 0.0)
        o["v"] = np.where(found, w[rows, best], 0.0)
    return out


def model_long(tri, points, prims=None):
    """(the smallest squared distance over all triangles, the squared distance to triangle prims[i]) of each
    point in np.longdouble, the geometric closest point without the clamp; NaN triangles ignored."""
    tri = np.asarray(tri, D).reshape(-1, 12)
    points = np.asarray(points, D).reshape(-1, 4)
    lo = np.zeros(len(points), np.longdouble)
    own = np.zeros(len(points), np.longdouble)
    step = max(1, cc.CHUNK // len(tri))
    for s in range(0, len(points), step):
        d2 = cc.pair_d2(tri, points[s:s + step], np.longdouble, clamp=False)[0]
        with np.errstate(all="ignore"):
            lo[s:s + step] = np.nanmin(d2, axis=1)
        if prims is not None:
            own[s:s + step] = d2[np.arange(d2.shape[0]), np.maximum(prims[s:s + step], 0)]
    return lo, own


def error_units(d2, d2_long, tri, points):
    """|d2 - d2_long| in units of eps M (sqrt(d2_long) + eps M), eps = 2^-53, M = max|point| + max|vertex|."""
    L = np.longdouble
    tri = np.asarray(tri, D).reshape(-1, 12)
    verts = np.stack([tri[:, 0:3], tri[:, 0:3] - tri[:, 3:6], tri[:, 0:3] + tri[:, 6:9]])
    M = L(np.abs(np.asarray(points, D)[:, :3]).max() + np.abs(verts).max())
    eps = L(2.0) ** -53
    return (np.abs(np.asarray(d2).astype(L) - d2_long) / (eps * M * (np.sqrt(d2_long) + eps * M))).astype(D)


# ---------------------------------------------------------------- the point sets
def vertices(tri):
    t = np.asarray(tri, D).reshape(-1, 12)
    return np.stack([t[:, 0:3], t[:, 0:3] - t[:, 3:6], t[:, 0:3] + t[:, 6:9]], axis=1)     # [tri, corner, xyz]


def base_sets(tri, seed=cc.SEED):
    """The sets (a) .. (d) and (f) of a mesh as closest_common.base_sets builds them, each [n, 4] float64 with
    r2max = +inf."""
    rng = np.random.default_rng(seed)
    v = vertices(tri)
    ok = np.isfinite(v).all(axis=(1, 2))
    v = v[ok] if ok.any() else v
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-300)
    sets = {}
    sets["a_uniform"] = centre + 1.5 * (hi - lo + 0.1 * ext) * (rng.random((PER_SET, 3)) - 0.5)
    pick = rng.integers(0, len(v), PER_SET)
    corner = rng.integers(0, 3, PER_SET)
    vert = v[pick, corner]
    mid = (v[pick, corner] + v[pick, (corner + 1) % 3]) * 0.5
    sets["b_on_mesh"] = np.concatenate([vert[: PER_SET // 2], mid[PER_SET // 2:]])
    sets["c_jitter"] = vert + 1e-3 * ext * rng.uniform(-1, 1, (PER_SET, 3))
    d = rng.normal(size=(PER_SET, 3))
    sets["d_far"] = centre + 40.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True)
    bad = sets["a_uniform"][:12].copy()
    for k, x in enumerate((np.nan, np.inf, -np.inf)):
        for j in range(3):
            bad[3 * k + j, j] = x
    bad[9] = [np.nan, np.nan, np.nan]
    bad[10] = [np.inf, -np.inf, 0]
    bad[11] = [np.inf, np.inf, np.inf]
    sets["f_nonfinite"] = bad
    return {k: np.concatenate([np.asarray(p, D), np.full((len(p), 1), np.inf, D)], axis=1) for k, p in sets.items()}


def radius_set(base, near):
    """Set (e): points of the base sets with a finite r2max -- 0, the model's own best d2 (still found), the
    double below it (a miss), a negative value, NaN."""
    keys = (("a_uniform", slice(0, 26)), ("b_on_mesh", slice(0, 26)), ("b_on_mesh", slice(-26, None)), ("c_jitter", slice(0, 26)),
            ("d_far", slice(0, 26)))
    pts = np.concatenate([base[k][s] for k, s in keys]).copy()
    best = np.concatenate([near[k][s] for k, s in keys])["d2"]
    r = np.empty(len(pts), D)
    r[0::5] = 0
    r[1::5] = best[1::5]
    r[2::5] = np.nextafter(best[2::5], 0.0)                           # best = 0: -denormal_min, still a miss
    r[2::5] = np.where(best[2::5] == 0, -5e-324, r[2::5])
    r[3::5] = -1
    r[4::5] = np.nan
    pts[:, 3] = r
    return pts


def sets_and_model(tri):
    """({name: points [n, 4]}, {name: the model's near32 records}) of a mesh, all six sets."""
    base = base_sets(tri)
    near = {k: model64_exact(tri, p) for k, p in base.items()}
    base["e_radius"] = radius_set(base, near)
    near["e_radius"] = model64_exact(tri, base["e_radius"])
    return base, near


joined = cc.joined


# ---------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def _scene(name, tmp):
    from conftest import import_package
    pkg = import_package()
    if name in cc.CONFIG:
        mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS[cc.CONFIG[name]], f64=True)
    else:
        mesh = pkg.load_obj_f64(dc.obj_path(name, tmp))
        bvh = pkg.build_bvh(mesh)
    return mesh, bvh


def scene(name, tmp=None):
    """(mesh, bvh) of the double of a closest_common scene; cap26 is written under `tmp` first."""
    return _scene(name, str(tmp) if name == "cap26" else None)


@functools.lru_cache(maxsize=None)
def _expected(name, tmp):
    mesh, _ = _scene(name, tmp)
    sets, near = sets_and_model(mesh.tri)
    for a in list(sets.values()) + list(near.values()):
        a.setflags(write=False)
    return sets, near


def expected(name, tmp=None):
    """(sets, model answers) of a scene, computed once and shared (read-only)."""
    return _expected(name, str(tmp) if name == "cap26" else None)


def moved_mesh(pkg, mesh, name):
    """closest_common.moved_mesh on the double mesh: power-of-two scalings, exact Tri96 records."""
    moved = cc.moved_mesh(pkg, mesh, name)
    assert moved.f64
    return moved


def overflow_mesh(pkg):
    """closest_common.overflow_mesh in double: beside two unit triangles, two of size 1e200 whose dot
    products overflow, so their d2 is NaN.  Such a triangle is never the answer."""
    tri = np.zeros((4, 12), D)
    tri[0, :9] = [0, 0, 0, -1, 0, 0, 0, 1, 0]
    tri[1, :9] = [1e200, 0, 0, 0, -1e200, 0, 0, 0, 1e200]
    tri[2, :9] = [0, 0, 1, 0, -1, 0, 1, 0, 0]
    tri[3, :9] = [-1e200, 1e200, 0, 1e200, 0, 0, 0, 0, -1e200]
    tri[:, 11] = 1
    return pkg.Mesh(tri, np.tile(np.asarray([0, 0, 1], D), (4, 3)))


def far_mesh(pkg, mesh, shift=FAR):
    """bunny_far: every p0 translated by `shift` (e1, e2 and the normals kept)."""
    tri = mesh.tri.copy()
    tri[:, 0:3] += shift
    return pkg.Mesh(tri, mesh.norm.copy())


def same(got, want):
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


def first_difference(got, want, points):
    g, w = np.asarray(got), np.asarray(want)
    bad = np.nonzero((g.view(np.uint64).reshape(-1, 4) != w.view(np.uint64).reshape(-1, 4)).any(axis=1))[0]
    if len(bad) == 0:
        return "equal"
    k = int(bad[0])
    return "%d of %d differ; first at %d: point %s got %s want %s" % (len(bad), len(g), k, points[k], g[k], w[k])
