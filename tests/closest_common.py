"""What the closest-point tests share (test_closest_cpu.py, test_gpu_closest.py): the numpy model that is
the oracle of both paths, the point sets, the scenes.

The contract (include/ceres_render.h, DESIGN.md "Closest-point queries") makes the answer the minimum over
ALL triangles of one float32 formula, ties to the smallest original index -- whatever the tree and the order
it is walked in.  model32 is that brute force, operation for operation; numpy's float32 + - * / are the
IEEE operations the library compiles, so the comparison is byte for byte.  model64 is the geometric closest
point in double, without the clamp, for the accuracy check."""
import functools
import os

import numpy as np

import deep_common as dc

F = np.float32
NEAR_DTYPE = np.dtype([("prim", np.int32), ("d2", np.float32), ("u", np.float32), ("v", np.float32)])
SCENES = ("tri1", "quad", "dupleaf", "degenerate", "bunny", "arms6", "bodyarms", "cap26")
CONFIG = {"tri1": "tri1", "quad": "quad", "dupleaf": "dupleaf", "degenerate": "degenerate", "bunny": "bunny_97x61_primary"}
SEED = 8100
PER_SET = 130                                                         # points of each set (a) .. (d)
CHUNK = 1 << 18                                                       # point-triangle pairs per numpy pass


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _min(x, y):
    return np.where(x < y, x, y)


def _max(x, y):
    return np.where(x > y, x, y)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def pair_d2(tri, pts, dt=F, clamp=True):
    """d2, v, w [points, triangles] of near_tri (closest_point.hpp) in the arithmetic `dt`: Ericson 5.1.5,
    his regions in his order, as a select chain from the last region to the first."""
    t = np.asarray(tri)[:, :9].astype(dt)
    p = np.asarray(pts)[:, :3].astype(dt)
    one, zero = dt(1), dt(0)
    a = [t[None, :, k] for k in range(3)]
    e1 = [t[None, :, 3 + k] for k in range(3)]
    e2 = [t[None, :, 6 + k] for k in range(3)]
    b = [a[k] - e1[k] for k in range(3)]
    c = [a[k] + e2[k] for k in range(3)]
    ab = [-e1[k] for k in range(3)]
    ac = e2
    P = [p[:, k, None] for k in range(3)]
    with np.errstate(all="ignore"):
        ap = [P[k] - a[k] for k in range(3)]
        bp = [P[k] - b[k] for k in range(3)]
        cp = [P[k] - c[k] for k in range(3)]
        d1, d2 = _dot(*ab, *ap), _dot(*ac, *ap)
        d3, d4 = _dot(*ab, *bp), _dot(*ac, *bp)
        d5, d6 = _dot(*ab, *cp), _dot(*ac, *cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        denom = one / ((va + vb) + vc)
        v, w = vb * denom, vc * denom                                 # interior
        m = (va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero)  # edge bc
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = np.where(m, one - wbc, v), np.where(m, wbc, w)
        m = (vb <= zero) & (d2 >= zero) & (d6 <= zero)                # edge ac
        v, w = np.where(m, zero, v), np.where(m, d2 / (d2 - d6), w)
        m = (d6 >= zero) & (d5 <= d6)                                 # vertex c
        v, w = np.where(m, zero, v), np.where(m, one, w)
        m = (vc <= zero) & (d1 >= zero) & (d3 <= zero)                # edge ab
        v, w = np.where(m, d1 / (d1 - d3), v), np.where(m, zero, w)
        m = (d3 >= zero) & (d4 <= d3)                                 # vertex b
        v, w = np.where(m, one, v), np.where(m, zero, w)
        m = (d1 <= zero) & (d2 <= zero)                               # vertex a
        v, w = np.where(m, zero, v), np.where(m, zero, w)
        v, w = v.astype(dt), w.astype(dt)
        d = []
        for k in range(3):
            q = (a[k] + ab[k] * v) + ac[k] * w
            if clamp:
                q = _clamp(q, _min(_min(a[k], b[k]), c[k]), _max(_max(a[k], b[k]), c[k]))
            d.append(P[k] - q)
        out = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return out, v, w


def model32(tri, points):
    """near16 records [n] of points [n, 4] float32 over tri [m, 12] (original order): the brute force with
    the selection rule -- best = r2max, a triangle replaces it iff d2 < best || (d2 == best && (none yet ||
    its index is smaller)); in index order that is: the smallest d2 <= r2max, the first index among equals."""
    tri = np.asarray(tri, F).reshape(-1, 12)
    points = np.asarray(points, F).reshape(-1, 4)
    out = np.zeros(len(points), NEAR_DTYPE)
    out["prim"] = -1
    step = max(1, CHUNK // len(tri))
    for s in range(0, len(points), step):
        pts = points[s:s + step]
        d2, v, w = pair_d2(tri, pts)
        with np.errstate(all="ignore"):
            ok = d2 <= pts[:, 3, None]                                # NaN d2, NaN or negative r2max: never
        key = np.where(ok, d2, F(np.inf))
        cand = ok & (key == key.min(axis=1, keepdims=True))           # (d2 = +inf <= r2max = +inf is a candidate too)
        best = cand.argmax(axis=1)                                    # the first index of the minimum
        rows = np.arange(len(pts))
        found = cand[rows, best]
        o = out[s:s + step]
        o["prim"] = np.where(found, best, -1)
        o["d2"] = np.where(found, d2[rows, best], F(0))
        o["u"] = np.where(found, v[rows, best], F(0))
        o["v"] = np.where(found, w[rows, best], F(0))
    return out


def model64(tri, points, prims=None):
    """(the smallest squared distance over all triangles, the squared distance to triangle prims[i]) of each
    point in float64, the geometric closest point without the clamp; NaN (degenerate) triangles ignored."""
    tri = np.asarray(tri, F).reshape(-1, 12)
    points = np.asarray(points, F).reshape(-1, 4)
    lo = np.zeros(len(points))
    own = np.zeros(len(points))
    step = max(1, CHUNK // len(tri))
    for s in range(0, len(points), step):
        d2 = pair_d2(tri, points[s:s + step], np.float64, clamp=False)[0]
        with np.errstate(all="ignore"):
            lo[s:s + step] = np.nanmin(d2, axis=1)
        if prims is not None:
            own[s:s + step] = d2[np.arange(d2.shape[0]), np.maximum(prims[s:s + step], 0)]
    return lo, own


def error_units(d2_32, d2_64, tri, points):
    """|d2_32 - d2_64| in units of eps M (sqrt(d2_64) + eps M), eps = 2^-24, M = max|point| + max|vertex|."""
    tri = np.asarray(tri, np.float64).reshape(-1, 12)
    verts = np.stack([tri[:, 0:3], tri[:, 0:3] - tri[:, 3:6], tri[:, 0:3] + tri[:, 6:9]])
    M = np.abs(np.asarray(points, np.float64)[:, :3]).max() + np.abs(verts).max()
    eps = 2.0 ** -24
    return np.abs(np.asarray(d2_32, np.float64) - d2_64) / (eps * M * (np.sqrt(d2_64) + eps * M))


# ---------------------------------------------------------------- the point sets
def vertices(tri):
    t = np.asarray(tri, F).reshape(-1, 12)
    return np.stack([t[:, 0:3], t[:, 0:3] - t[:, 3:6], t[:, 0:3] + t[:, 6:9]], axis=1)     # [tri, corner, xyz]


def base_sets(tri, seed=SEED):
    """The sets (a) .. (d) and (f) of a mesh, each [n, 4] float32 with r2max = +inf."""
    rng = np.random.default_rng(seed)
    v = vertices(tri)
    ok = np.isfinite(v).all(axis=(1, 2))
    v = v[ok] if ok.any() else v
    lo, hi = v.reshape(-1, 3).min(0).astype(np.float64), v.reshape(-1, 3).max(0).astype(np.float64)
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-30)
    sets = {}
    sets["a_uniform"] = centre + 1.5 * (hi - lo + 0.1 * ext) * (rng.random((PER_SET, 3)) - 0.5)
    pick = rng.integers(0, len(v), PER_SET)
    corner = rng.integers(0, 3, PER_SET)
    vert = v[pick, corner]
    mid = ((v[pick, corner] + v[pick, (corner + 1) % 3]) * F(0.5)).astype(F)
    sets["b_on_mesh"] = np.concatenate([vert[: PER_SET // 2], mid[PER_SET // 2:]])
    sets["c_jitter"] = vert.astype(np.float64) + 1e-3 * ext * rng.uniform(-1, 1, (PER_SET, 3))
    d = rng.normal(size=(PER_SET, 3))
    sets["d_far"] = centre + 40.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True)
    bad = sets["a_uniform"][:12].astype(F).copy()
    for k, x in enumerate((np.nan, np.inf, -np.inf)):
        for j in range(3):
            bad[3 * k + j, j] = x
    bad[9] = [np.nan, np.nan, np.nan]
    bad[10] = [np.inf, -np.inf, 0]
    bad[11] = [np.inf, np.inf, np.inf]
    sets["f_nonfinite"] = bad
    return {k: np.concatenate([np.asarray(p, F), np.full((len(p), 1), np.inf, F)], axis=1) for k, p in sets.items()}


def radius_set(base, near):
    """Set (e): points of the base sets with a finite r2max -- 0, the model's own best d2 (still found), the
    float below it (a miss), a negative value, NaN."""
    pts = np.concatenate([base["a_uniform"][:26], base["b_on_mesh"][:26], base["b_on_mesh"][-26:], base["c_jitter"][:26],
                          base["d_far"][:26]]).copy()
    best = np.concatenate([near["a_uniform"][:26], near["b_on_mesh"][:26], near["b_on_mesh"][-26:], near["c_jitter"][:26],
                           near["d_far"][:26]])["d2"]
    r = np.empty(len(pts), F)
    r[0::5] = 0
    r[1::5] = best[1::5]
    r[2::5] = np.nextafter(best[2::5], F(0))                          # best = 0: -denormal_min, still a miss
    r[2::5] = np.where(best[2::5] == 0, F(-1e-45), r[2::5])
    r[3::5] = -1
    r[4::5] = np.nan
    pts[:, 3] = r
    return pts


ORDER = ("a_uniform", "b_on_mesh", "c_jitter", "d_far", "e_radius", "f_nonfinite")


def sets_and_model(tri):
    """({name: points [n, 4]}, {name: the model's near16 records}) of a mesh, all six sets."""
    base = base_sets(tri)
    near = {k: model32(tri, p) for k, p in base.items()}
    base["e_radius"] = radius_set(base, near)
    near["e_radius"] = model32(tri, base["e_radius"])
    return base, near


def joined(d):
    return np.concatenate([d[k] for k in ORDER])


# ---------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def _scene(name, tmp):
    from conftest import import_package
    pkg = import_package()
    if name in CONFIG:
        mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS[CONFIG[name]])
    else:
        mesh = pkg.load_obj(dc.obj_path(name, tmp))
        bvh = pkg.build_bvh(mesh)
    return mesh, bvh


def scene(name, tmp=None):
    """(mesh, bvh) of a scene; cap26 is written under `tmp` first."""
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
    """The mesh after a move a refit can follow: the deep meshes' own (deep_common.moved); else every third
    triangle (from the second) scaled by 1/2 about the origin and every fifth (from the third) by 2 (powers of two: exact Tri48 records)."""
    if name in dc.MESHES:
        return dc.moved(pkg, mesh, name)
    tri = mesh.tri.copy()
    for first, step, f in ((1, 3, F(0.5)), (2, 5, F(2.0))):
        tri[first::step, :9] *= f
        tri[first::step, 9:] *= f * f
    return pkg.Mesh(tri, mesh.norm.copy())


def overflow_mesh(pkg):
    """Finite coordinates whose d2 is NaN: beside two unit triangles, two of size 1e20 -- their dot products
    overflow to inf, va / vb / vc become inf - inf, every region test fails and the interior branch gives
    NaN.  Such a triangle is never the answer."""
    tri = np.zeros((4, 12), F)
    tri[0, :9] = [0, 0, 0, -1, 0, 0, 0, 1, 0]
    tri[1, :9] = [1e20, 0, 0, 0, -1e20, 0, 0, 0, 1e20]
    tri[2, :9] = [0, 0, 1, 0, -1, 0, 1, 0, 0]
    tri[3, :9] = [-1e20, 1e20, 0, 1e20, 0, 0, 0, 0, -1e20]
    tri[:, 11] = 1
    return pkg.Mesh(tri, np.tile(np.asarray([0, 0, 1], F), (4, 3)))


def same(got, want):
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


def first_difference(got, want, points):
    g, w = np.asarray(got), np.asarray(want)
    bad = np.nonzero((g.view(np.uint32).reshape(-1, 4) != w.view(np.uint32).reshape(-1, 4)).any(axis=1))[0]
    if len(bad) == 0:
        return "equal"
    k = int(bad[0])
    return "%d of %d differ; first at %d: point %s got %s want %s" % (len(bad), len(g), k, points[k], g[k], w[k])


def write_points(path, points):
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(points, F).tobytes())
    return os.fspath(path)
