"""Shared by tests/test_quality_cpu.py and tests/test_gpu_quality.py: a numpy model of the SAH cost the
upkeep calls report (ceres_scene_sah_cost, the `cost` fields of ceres_update_info) and the inputs of a case.

Expected values come from code the feature does not touch: `model_cost` evaluates the definition in numpy
float64 on REFERENCE-LAYOUT nodes -- `pkg.build_bvh(...)` output or `refit_common.refit_nodes(...)` -- never
on a scene's own records.  The cost is a sum over nodes, so node numbering does not matter.

The definition (sah_based_algorithm.hpp:21-32 with traversal_cost = 1): HA(box) = (d0 + d1) * d2 + d0 * d1
with d = hi - lo (bounding_box.hpp:43-46), in double on the stored bounds; ROOT = the union of the root's
two child boxes; cost = (HA(ROOT) + sum over every non-root node of HA(node) * w) / HA(ROOT), w = the
triangle count of a leaf and 1 for an inner node; a root leaf costs its triangle count."""
import functools

import numpy as np

import refit_common as rc


def half_area(b):
    b = np.asarray(b, np.float64)
    d0, d1, d2 = b[..., 1] - b[..., 0], b[..., 3] - b[..., 2], b[..., 5] - b[..., 4]
    return (d0 + d1) * d2 + d0 * d1


def model_cost(nodes):
    """The SAH cost of reference-layout nodes ([m, 8] uint32 / uint64), walked from the root."""
    bounds, count, first = rc.node_fields(nodes)
    if count[0]:
        return float(count[0])
    kids = bounds[first[0]:first[0] + 2].astype(np.float64)
    root = np.empty(6)
    root[0::2] = kids[:, 0::2].min(axis=0)
    root[1::2] = kids[:, 1::2].max(axis=0)
    total = 0.0
    frontier = np.array([0], np.int64)
    while frontier.size:
        c = np.concatenate([first[frontier], first[frontier] + 1])
        w = np.where(count[c] > 0, count[c], 1).astype(np.float64)
        total += float(np.sum(half_area(bounds[c]) * w))
        frontier = c[count[c] == 0]
    ha = float(half_area(root))
    return (ha + total) / ha


def tolerance(nodes):
    """Relative bound of any evaluation of the definition against another: every term is non-negative, so
    any summation order of n terms, the few roundings per term and the final division stay within
    (n + 16) * 2**-52, n the node count."""
    return (nodes.shape[0] + 16) * 2.0 ** -52


def assert_cost(got, nodes, what=""):
    want = model_cost(nodes)
    print("%s cost %.17g model %.17g rel %.3g bound %.3g" % (what, got, want, abs(got - want) / want, tolerance(nodes)))
    assert abs(got - want) <= tolerance(nodes) * want, (what, got, want)


def dbits(x):
    return np.float64(x).tobytes()


@functools.lru_cache(maxsize=None)
def inputs(name, f64=False, arith=0):
    """One case's meshes and reference-layout BVHs: as built, refitted to MOVE (numpy), rebuilt for MOVE
    (the host builder), and that rebuilt tree refitted to OTHER; r = the model's cost ratio of the MOVE
    refit, which the update thresholds are derived from."""
    from conftest import import_package
    pkg = import_package()
    mesh, bvh, moved, moved_bvh = rc.moved_scene_inputs(pkg, name, f64, arith)
    rebuilt_bvh = pkg.build_bvh(moved, arith)
    other = rc.deform(mesh, **rc.OTHER)
    other_bvh = pkg.Bvh(rc.refit_nodes(rebuilt_bvh.nodes, rebuilt_bvh.prim, other.tri), rebuilt_bvh.prim)
    basis, sun, W, H, mode = rc.pose_of(pkg, name, f64, arith)
    r = model_cost(moved_bvh.nodes) / model_cost(bvh.nodes)
    return dict(mesh=mesh, bvh=bvh, moved=moved, moved_bvh=moved_bvh, rebuilt_bvh=rebuilt_bvh, other=other,
                other_bvh=other_bvh, basis=basis, sun=sun, W=W, H=H, mode=mode, r=r)
