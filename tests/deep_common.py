"""Meshes whose reference BVH is 40 to 64 levels deep, from a few hundred triangles.

An "arm" is a row of triangles along a direction d: triangle k sits at s_k d and is about s_k = ratio^k
large, so every SAH split peels off the largest triangle or two and the tree is a chain -- the shape
a small, finely modelled spacecraft beside a body orders of magnitude larger gives, or a mesh whose
tessellation shrinks towards a landing site.  Everything is scaled by 2^30 (a power of two: the trees
are those of the unscaled recipe) so that n.n of the smallest triangle does not underflow to zero
and no shading NaN arises (measured: 1.05e-38 for arms6 and bodyarms, 9.1e-41 for cap26 -- subnormal
floats, which the kernels do not flush).

  arms6     arms(60, .5, SIX)                          360 triangles
  bodyarms  an icosphere (2 subdivisions), then arms6  680 triangles
  cap26     arms(100, .66, D26)                        2600 triangles, the reference's depth cap (64)

arms6 and bodyarms are committed as OBJ text under tests/golden/ (test_deep_cpu.py holds the files
to this generator byte for byte); cap26 is generated when a test needs it and held to its sha256;
the reference's answers on it are tests/golden/deep/cap26.json (tests/golden/make_golden_deep.py)."""
import functools
import hashlib
import itertools
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALE = 2.0 ** 30
SIX = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
D26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
CAP26_SHA256 = "a708da39afb78e93929f8943b3a7307947bc21ee9f63ed82065d56ac3ee897bd"


def arms(n, ratio, dirs, jit=0.2, seed=5, scale=SCALE):
    rng = np.random.default_rng(seed)
    out = []
    for d in dirs:
        s = ratio ** np.arange(n)
        c = s[:, None] * np.asarray(d, float)[None, :]
        out.append(c[:, None, :] + s[:, None, None] * jit * rng.uniform(-1, 1, (n, 3, 3)))
    return (np.concatenate(out) * scale).astype(np.float32)      # [tri, corner, xyz]


def icosphere(subdiv=2, radius=0.5, centre=(2.0, 2.0, 2.0), scale=SCALE):
    """[tri, corner, xyz] of a subdivided icosahedron, outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    tri = np.asarray(v, float)[np.asarray(f)]
    tri /= np.linalg.norm(tri, axis=2, keepdims=True)
    for _ in range(subdiv):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        tri = np.concatenate([np.stack(q, axis=1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return ((tri * radius + np.asarray(centre, float)) * scale).astype(np.float32)


def arms6():
    return arms(60, .5, SIX)


def bodyarms():
    return np.concatenate([icosphere(), arms(60, .5, SIX)])


def cap26():
    return arms(100, .66, D26)


def arm1():
    """One arm alone, 64 triangles shrinking by 0.35: a tree of 36 levels that the 64-node entry cut opens
    completely, its deepest LCA at depth 35 (measured, both arithmetics; at ratio 0.5 the binned SAH
    splits off several triangles at once and the chain is 26 deep)."""
    return arms(64, .35, SIX[:1])


MESHES = {"arms6": arms6, "bodyarms": bodyarms, "cap26": cap26}


def obj_text(tri):
    """One `v` per corner, one `f` per triangle, no shared vertices."""
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    lines = ["v %.9g %.9g %.9g" % tuple(float(x) for x in c) for c in tri.reshape(-1, 3)]
    lines += ["f %d %d %d" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(len(tri))]
    return ("\n".join(lines) + "\n").encode()


def obj_path(name, tmp=None):
    """The committed file of arms6 / bodyarms; cap26 written under `tmp` (and held to its sha256)."""
    if name != "cap26":
        return os.path.join(GOLDEN, name + ".obj")
    text = obj_text(cap26())
    assert hashlib.sha256(text).hexdigest() == CAP26_SHA256, "cap26 is not the mesh its fixture was made from"
    p = os.path.join(str(tmp), "cap26.obj")
    with open(p, "wb") as f:
        f.write(text)
    return p


# cap26's views: (zoom, W, H, mode) -- the deep configs' camera (configs._deep) at 2^-zoom
CAP26_VIEWS = {"full": (8, 136, 72, "full"), "zoom": (32, 97, 61, "full"), "primary": (8, 136, 72, "primary")}


def cap26_cfg(view, obj):
    """A config dict (as configs.CONFIGS holds them) of one cap26 view over the OBJ file `obj`."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ceres-raytracer_amd"))
    import configs
    zoom, W, H, mode = CAP26_VIEWS[view]
    cfg = configs._deep("cap26", configs._ARM_EYE, zoom, W=W, H=H, mode=mode)
    cfg["obj"] = obj                                                  # absolute: configs.obj_path keeps it
    return cfg


@functools.lru_cache(maxsize=None)
def load_cap26():
    with open(os.path.join(GOLDEN, "deep", "cap26.json")) as f:
        return json.load(f)


def bits(hexes):
    return np.asarray([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def check_view(prim, shadow, mode="full"):
    """A view is worth rendering: the reference hits a tenth of the pixels and eight primitives, and
    (full mode) finds lit and shadowed pixels."""
    prim, shadow = np.asarray(prim), np.asarray(shadow)
    hit = prim >= 0
    assert 10 * np.count_nonzero(hit) >= hit.size, "hits on %d of %d pixels" % (np.count_nonzero(hit), hit.size)
    assert len(np.unique(prim[hit])) >= 8
    if mode == "full":
        assert (shadow == 0).any() and (shadow == 1).any()


def depth_and_leaf(nodes):
    """(levels of inner nodes on the longest root-leaf path -- Scene.info()'s depth --, largest leaf)."""
    nd = np.asarray(nodes).reshape(-1, 8)
    cnt, first = nd[:, 6], nd[:, 7]
    if cnt[0]:
        return 0, int(cnt[0])
    depth, st = 0, [(0, 1)]
    while st:
        x, lvl = st.pop()
        depth = max(depth, lvl)
        c = int(first[x])
        st += [(s, lvl + 1) for s in (c, c + 1) if cnt[s] == 0]
    return depth, int(cnt.max())


def moved(pkg, mesh, name):
    """The mesh with arm a scaled by 2^(a mod 5 - 2) about the origin, the icosphere kept.  Powers of
    two: p0, e1, e2 scale exactly and n = cross(e1, e2) by the square, in either arithmetic, so the
    Tri48 records are those a loader would compute from the moved corners."""
    tri = mesh.tri.copy()
    n_arm, dirs = (100, len(D26)) if name == "cap26" else (60, 6)
    base = len(tri) - n_arm * dirs
    for a in range(dirs):
        f = np.float32(2.0 ** (a % 5 - 2))
        tri[base + a * n_arm: base + (a + 1) * n_arm, :9] *= f
        tri[base + a * n_arm: base + (a + 1) * n_arm, 9:] *= f * f
    return pkg.Mesh(tri, mesh.norm.copy())
