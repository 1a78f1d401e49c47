"""Shared by tests/test_refit_cpu.py and tests/test_gpu_refit.py: a numpy model of the refit semantics and
the deformation the tests move the meshes with.

Every refit test compares a REFITTED scene with a FRESH scene that the existing constructors create from
the moved triangles and a BVH refitted here, in numpy, on the reference-layout nodes -- code the feature
does not touch.  Both scenes consume the same arrays, so no reference arithmetic is involved: only min / max.

The semantics (hierarchy_refitter.hpp:17-32 with the usual leaf update): a leaf's box is the union over its
triangles of Triangle::bounding_box() (triangle.hpp:36-44: p0, p0 - e1, p0 + e2, in the scene's scalar
type), an inner node's box the union of its two children's (bounding_box.hpp:23-26)."""
import numpy as np

from conftest import import_package

SCENES = ["bunny_orbit7_160x120", "quad", "tri1", "dupleaf"]

# deformation constants (in units of the mesh's largest half extent), chosen on the CPU path with the
# fresh scene alone so that, for every scene of SCENES at its config's pose, the deformed frame differs
# from the undeformed one, has primary hits on at least a tenth of the pixels and -- where the
# undeformed scene casts shadows on itself at all (bunny, dupleaf) -- shows lit and occluded pixels
# (measured at these constants: hits on 0.81 / 0.76 / 0.15 / 0.99 of the pixels of bunny / quad / tri1 /
# dupleaf; the lone triangle of tri1 needs the enlargement to reach a tenth); the scale and the shift
# move part of the body outside the old root box (test_refit_cpu.py asserts all of it)
MOVE = dict(twist=0.9, bend=0.25, scale=(2.6, 1.9, 2.5), shift=(0.45, 0.15, -0.1))
# "deformed again with other constants": the second refit of the two-refits test
OTHER = dict(twist=-0.5, bend=-0.2, scale=(2.0, 2.4, 1.9), shift=(-0.3, -0.1, 0.15))


def node_fields(nodes):
    """(bounds [m, 6] float view, count [m], first [m]) of reference-layout nodes: [m, 8] uint32
    (Bvh<float>::Node) or uint64 (Bvh<double>::Node)."""
    f = np.float64 if nodes.dtype == np.uint64 else np.float32
    return nodes[:, :6].view(f), nodes[:, 6].astype(np.int64), nodes[:, 7].astype(np.int64)


def lesser(a, b):
    """std::min(a, b) elementwise: b where b < a, else a -- a NaN in b is dropped, one in a stays."""
    with np.errstate(invalid="ignore"):
        return np.where(b < a, b, a)


def greater(a, b):
    """std::max(a, b) elementwise: b where a < b, else a."""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a)


def tri_boxes(tri):
    """Per triangle, [n, 6] in the bvh.hpp:25-30 order, in tri's dtype: the empty box (+inf, -inf) extended
    by p0, p0 - e1 and p0 + e2 in that order with std::min / std::max (bounding_box.hpp:23-27), as the refit
    does.  A NaN coordinate always arrives second and is dropped, so no box holds a NaN; a triangle whose
    three points are NaN on an axis leaves that axis empty."""
    p0, e1, e2 = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    out = np.empty((tri.shape[0], 6), tri.dtype)
    lo = np.full(p0.shape, np.inf, tri.dtype)
    hi = np.full(p0.shape, -np.inf, tri.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        pts = (p0, p0 - e1, p0 + e2)
    for p in pts:
        lo, hi = lesser(lo, p), greater(hi, p)
    out[:, 0::2] = lo
    out[:, 1::2] = hi
    return out


def refit_nodes(nodes, prim, tri):
    """The refitted copy of `nodes` for the moved triangles `tri` (original order): one reverse-index
    pass, which needs every child after its parent -- asserted.  An inner node's box is std::min / std::max
    of (left child, right child) in that order (hierarchy_refitter.hpp:27-30); a leaf's the union of its
    triangles' boxes, which hold no NaN (tri_boxes), so numpy's min / max give the sequential fold's values."""
    out = nodes.copy()
    bounds, count, first = node_fields(out)
    tb = tri_boxes(np.ascontiguousarray(tri, bounds.dtype))
    prim = np.asarray(prim, np.int64)
    inner = count == 0
    assert np.all(first[inner] > np.flatnonzero(inner)), "fixture: a child numbered before its parent"
    for k in range(out.shape[0] - 1, -1, -1):
        if count[k]:
            b = tb[prim[first[k]:first[k] + count[k]]]
            bounds[k, 0::2] = b[:, 0::2].min(axis=0)
            bounds[k, 1::2] = b[:, 1::2].max(axis=0)
        else:
            l, r = bounds[first[k]], bounds[first[k] + 1]
            bounds[k, 0::2] = lesser(l[0::2], r[0::2])
            bounds[k, 1::2] = greater(l[1::2], r[1::2])
    return out


def box_set(nodes):
    """The refitted boxes as a set of 6-tuples (for membership tests of BVH4 child boxes)."""
    bounds, _, _ = node_fields(nodes)
    return {tuple(float(x) for x in row) for row in bounds}


def deform(mesh, twist=MOVE["twist"], bend=MOVE["bend"], scale=MOVE["scale"], shift=MOVE["shift"]):
    """The mesh moved: its vertices p0, p0 - e1, p0 + e2 twisted about y by an angle proportional to y,
    bent with a sine of x, scaled non-uniformly and shifted, all in float64 in units of the mesh's largest
    half extent, then rounded to the mesh's scalar type; {p0, e1 = p0 - p1, e2 = p2 - p0, n = cross(e1,
    e2)} rebuilt in that type with numpy.  The vertex normals move too (blended with the new face
    normal), so stale normals show."""
    pkg = import_package()
    S = mesh.tri.dtype
    t = mesh.tri.astype(np.float64)
    p0 = t[:, 0:3]
    V = np.stack([p0, p0 - t[:, 3:6], p0 + t[:, 6:9]], axis=1)            # [n, 3 vertices, 3]
    lo, hi = V.min(axis=(0, 1)), V.max(axis=(0, 1))
    c, ext = (lo + hi) / 2, float(np.max(hi - lo) / 2) or 1.0
    q = (V - c) / ext
    ang = twist * q[..., 1]
    x = np.cos(ang) * q[..., 0] + np.sin(ang) * q[..., 2]
    z = -np.sin(ang) * q[..., 0] + np.cos(ang) * q[..., 2]
    y = q[..., 1] + bend * np.sin(3.0 * x)
    q = np.stack([x, y, z], axis=-1) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    W = (c + ext * q).astype(S)
    P0, P1, P2 = W[:, 0], W[:, 1], W[:, 2]
    e1, e2 = P0 - P1, P2 - P0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    tri = np.concatenate([P0, e1, e2, n], axis=1).astype(S)
    old = mesh.norm.astype(np.float64).reshape(-1, 3, 3)
    ln = np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)
    flat = np.where(ln > 0, n.astype(np.float64) / np.where(ln > 0, ln, 1), 0.0)
    new = old + flat[:, None, :]
    l2 = np.linalg.norm(new, axis=2, keepdims=True)
    new = np.where(l2 > 0, new / np.where(l2 > 0, l2, 1), old)
    return pkg.Mesh(tri, new.reshape(-1, 9).astype(S))


def moved_scene_inputs(pkg, name, f64=False, arith=0, **constants):
    """(mesh, bvh, moved mesh, refitted Bvh for the moved mesh) of a config."""
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS[name], f64=f64, arith=arith)
    moved = deform(mesh, **constants) if constants else deform(mesh)
    return mesh, bvh, moved, pkg.Bvh(refit_nodes(bvh.nodes, bvh.prim, moved.tri), bvh.prim)


def pose_of(pkg, name, f64=False, arith=0):
    """(basis12, sun, W, H, mode) of a config in the scene's scalar type."""
    cfg = pkg.configs.CONFIGS[name]
    cam, sun = pkg.pose_f64(cfg, arith) if f64 else pkg.pose(cfg, arith=arith)
    return cam.basis(cfg["W"], cfg["H"]), sun, cfg["W"], cfg["H"], pkg.cfg_mode(cfg, arith)


def write_obj(path, mesh):
    """A tiny OBJ writer: three `v` lines and one `f -3 -2 -1` line per triangle, coordinates printed so
    that strtof reads the float32 values back."""
    t = mesh.tri.astype(np.float32)
    with open(path, "w") as f:
        for p0, e1, e2 in zip(t[:, 0:3], t[:, 3:6], t[:, 6:9]):
            for v in (p0, p0 - e1, p0 + e2):
                f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in v))
            f.write("f -3 -2 -1\n")
