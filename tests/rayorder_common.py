"""Shared pieces of the coherent-ray-order and indexed-query tests (test_rayorder_cpu.py,
test_gpu_indexed.py): a numpy transcription of the order's key (ray_key.hpp: the same IEEE operations
in the same order, on float32 or float64 arrays), the order that follows from it, the ray sets the
issue names, and builders of index lists."""
import functools

import numpy as np

import allhits64_common as a64
import allhits_common as ac
import trace64_common as t64
import trace_common as tc
from conftest import import_package

DEAD = np.uint32(0x80000000)
GRID = 128
FLOAT_SETS = ["dragon_adversarial", "tri1_tiny", "quad_tiny", "lattice_ties", "soup_nan_p0_300"]
DOUBLE_SETS = ["dragon_adversarial64", "tri1_tiny64", "quad_tiny64", "lattice_ties64"]
PREFIXES = (0, 1, 63, 64, 65)


def set_scene(name):
    """(mesh, bvh) of a set's scene in the exact arithmetic."""
    return t64.ray_set_scene(name) if name.endswith("64") else ac.all_set_scene(name, 0)


@functools.lru_cache(maxsize=None)
def set_rays(name):
    """The stored rays of a set: float32 [n, 8], or float64 for the rays64 sets."""
    rays = t64.load_ray_fixture64(name)["rays"] if name.endswith("64") else ac.load_all_fixture(name)["rays"]
    return np.ascontiguousarray(rays)


def order_box(mesh, bvh):
    """The key's box from the scene's own data, independent of the library: the union of the boxes of the
    root's two children, usable when the root is inner and the six numbers are finite with lo <= hi.
    Returns (lo [3], hi [3], usable) in the mesh's precision."""
    dt = np.float64 if mesh.f64 else np.float32
    nodes = np.ascontiguousarray(bvh.nodes)
    stride = nodes.shape[1] * nodes.dtype.itemsize
    raw = nodes.view(np.uint8).reshape(nodes.shape[0], stride)
    nb = 6 * np.dtype(dt).itemsize
    bounds = np.ascontiguousarray(raw[:, :nb]).view(dt).reshape(-1, 6)
    tail = np.ascontiguousarray(raw[:, nb:nb + 16]).view(np.uint64 if mesh.f64 else np.uint32).reshape(nodes.shape[0], -1)
    count, first = int(tail[0, 0]), int(tail[0, 1])
    if count != 0:                                                    # the root is a leaf
        return np.zeros(3, dt), np.zeros(3, dt), False
    l, r = bounds[first], bounds[first + 1]
    with np.errstate(all="ignore"):
        lo = np.where(l[0::2] < r[0::2], l[0::2], r[0::2]).astype(dt)
        hi = np.where(l[1::2] > r[1::2], l[1::2], r[1::2]).astype(dt)
        ok = bool(np.isfinite(l).all() and np.isfinite(r).all() and (lo <= hi).all())
    return lo, hi, ok


def _spread7(c):
    m = np.zeros_like(c)
    for i in range(7):
        m |= ((c >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i)
    return m


def model_keys(rays, lo, hi, usable):
    """ray_key.hpp on arrays: rays [n, 8] float32 / float64, the box in the same dtype."""
    dt = rays.dtype.type
    n = len(rays)
    o, d, tmin, tmax = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with np.errstate(all="ignore"):
        dead = ~(tmin <= tmax)
        dead |= ~np.isfinite(o).all(axis=1) | ~np.isfinite(d).all(axis=1)
        dead |= (d == 0).all(axis=1)
        cell = np.zeros((n, 3), np.uint32)
        if usable:
            t0, t1 = tmin.copy(), tmax.copy()
            empty = np.zeros(n, bool)
            for a in range(3):
                zero = d[:, a] == 0
                empty |= zero & ~((lo[a] <= o[:, a]) & (o[:, a] <= hi[a]))
                ta = (lo[a] - o[:, a]) / d[:, a]
                tb = (hi[a] - o[:, a]) / d[:, a]
                tn, tf = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
                t0 = np.where(~zero & (tn > t0), tn, t0)
                t1 = np.where(~zero & (tf < t1), tf, t1)
            dead |= empty | ~(t0 <= t1)
            for a in range(3):
                ext = dt(hi[a] - lo[a])
                if not ext > 0:
                    continue
                p = o[:, a] + t0 * d[:, a]
                f = (p - lo[a]) / ext * dt(GRID)
                assert f.dtype == rays.dtype
                c = np.where(f >= dt(GRID - 1), dt(GRID - 1), f)
                c = np.where(f >= 0, c, dt(0))                         # below the box or NaN: cell 0
                cell[:, a] = c.astype(np.uint32)                       # truncates
    sign = (np.signbit(d[:, 0]).astype(np.uint32) | (np.signbit(d[:, 1]).astype(np.uint32) << np.uint32(1))
            | (np.signbit(d[:, 2]).astype(np.uint32) << np.uint32(2)))
    morton = _spread7(cell[:, 0]) | (_spread7(cell[:, 1]) << np.uint32(1)) | (_spread7(cell[:, 2]) << np.uint32(2))
    keys = (sign << np.uint32(28)) | (morton << np.uint32(7))
    return np.where(dead, DEAD, keys).astype(np.uint32)


def model_order(rays, lo, hi, usable):
    return np.argsort(model_keys(rays, lo, hi, usable), kind="stable").astype(np.uint32)


def set_model_order(name, n=None):
    rays = set_rays(name)[:n]
    return model_order(rays, *order_box(*set_scene(name)))


# ---- index lists
def every_third(n_rays):
    return np.arange(0, n_rays, 3, dtype=np.uint32)


def subset_with_bad_entries(n_rays, length, seed=7):
    """`length` entries: every third ray (cycled when the set is short), then -- where there is room --
    the invalid entries n_rays, n_rays + 1 and 0xffffffff and one duplicate, at fixed pseudo-random places."""
    base = np.resize(every_third(n_rays), length).astype(np.uint32)
    if length >= 8:
        rng = np.random.default_rng(seed + length)
        at = rng.choice(length, 5, replace=False)
        base[at[0]], base[at[1]], base[at[2]] = n_rays, n_rays + 1, 0xffffffff
        base[at[3]] = base[at[4]]                                     # the duplicate (of a valid entry)
    return base


def valid_rays(index, n_rays):
    """The distinct rays a list traces."""
    return np.unique(index[index < n_rays])


def random_permutation(n, seed=20261021):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


# ---- coherence
def hit_groups(hit, seq):
    """Groups of 64 consecutive rays of `seq` with at least one hit ray; (count, groups)."""
    h = hit[seq]
    pad = (-len(h)) % 64
    g = np.concatenate([h, np.zeros(pad, bool)]).reshape(-1, 64)
    return int(g.any(axis=1).sum()), len(g)


def dragon_view_rays():
    """(rays, mesh, bvh): the camera rays of the dragon 333 x 217 view, shuffled with a fixed seed."""
    pkg = import_package()
    cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(tc.DRAGON, 0)
    rays = pkg.camera_rays(basis, cfg["W"], cfg["H"])
    return np.ascontiguousarray(rays[random_permutation(len(rays), 333217)]), mesh, bvh
