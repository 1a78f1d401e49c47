"""The coherent ray order on the host (ceres_ray_order_cpu / _f64, CpuScene.ray_order) and the host
arithmetic of ceres_ray_order_scratch_bytes.  No GPU: the order is pinned to a numpy transcription of
the key (rayorder_common.model_keys) entry for entry, and a floor shows that the key does something."""
import ctypes

import numpy as np
import pytest

import rayorder_common as ro
import trace_common as tc


@pytest.fixture(scope="module")
def cpu_scenes(pkg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pkg.CpuScene(*ro.set_scene(name))
        return cache[name]

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("name", ro.FLOAT_SETS + ro.DOUBLE_SETS)
def test_cpu_order_equals_the_numpy_model(pkg, cpu_scenes, name):
    """CpuScene.ray_order is the stable argsort of the model keys, exactly, and a permutation; so are the
    prefixes of 0, 1, 63, 64 and 65 rays."""
    rays = ro.set_rays(name)
    mesh, bvh = ro.set_scene(name)
    lo, hi, usable = ro.order_box(mesh, bvh)
    blo, bhi, busable = cpu_scenes(name).order_box()
    assert busable == usable, name
    if usable:
        assert np.array_equal(blo, lo.astype(np.float64)) and np.array_equal(bhi, hi.astype(np.float64)), name
    for n in ro.PREFIXES + (len(rays),):
        got = cpu_scenes(name).ray_order(rays[:n])
        assert got.dtype == np.uint32 and got.shape == (n,)
        assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32)), (name, n, "not a permutation")
        exp = ro.model_order(rays[:n], lo, hi, usable)
        assert np.array_equal(got, exp), (name, n, "first differing place", np.flatnonzero(got != exp)[:4])


def test_the_sets_reach_the_keys_cases(pkg):
    """The inputs' own conditions: dead and live rays, several octants and cells on the dragon; the
    smallest usable box on the quad; no usable box on tri1 (a root that is a leaf: every cell is 0)."""
    rays = ro.set_rays("dragon_adversarial")
    keys = ro.model_keys(rays, *ro.order_box(*ro.set_scene("dragon_adversarial")))
    live = keys[keys != ro.DEAD]
    assert (keys == ro.DEAD).sum() >= 64 and len(live) >= 512              # several wavefronts of each kind
    assert len(np.unique(live >> np.uint32(28))) == 8 and len(np.unique((live >> np.uint32(7)) & np.uint32((1 << 21) - 1))) >= 64
    assert ro.order_box(*ro.set_scene("quad_tiny"))[2]                 # two leaves under an inner root: a usable box
    assert not ro.order_box(*ro.set_scene("tri1_tiny"))[2]
    k = ro.model_keys(ro.set_rays("tri1_tiny"), *ro.order_box(*ro.set_scene("tri1_tiny")))
    assert not ((k[k != ro.DEAD] >> np.uint32(7)) & np.uint32((1 << 21) - 1)).any()


def test_dead_rays_among_the_reference_hits_are_reported(pkg):
    """A quality figure, printed and not asserted (the plain slab test is not conservative, and a dead mark
    can cost time only): the rays with a stored reference hit (any of the four variants) that the key marks
    dead.  Asserted is only that the key of a hit ray is a key: dead exactly, or with its low 7 bits clear."""
    for name in ("dragon_adversarial", "quad_tiny", "lattice_ties"):
        fx = tc.load_ray_fixture(name)
        keys = ro.model_keys(ro.set_rays(name), *ro.order_box(*ro.set_scene(name)))
        hit = np.zeros(len(keys), bool)
        for v in tc.RAY_VARIANTS:
            hit |= fx[v]["prim"] >= 0
        n = int((hit & (keys == ro.DEAD)).sum())
        print("%s: %d of %d reference-hit rays marked dead" % (name, n, int(hit.sum())))
        k = keys[hit]
        assert (((k & np.uint32(0x7f)) == 0) | (k == ro.DEAD)).all() and ((k < ro.DEAD) | (k == ro.DEAD)).all(), name


def test_refusals(pkg, cpu_scenes):
    L = pkg.lib()
    f32, f64 = cpu_scenes("quad_tiny"), cpu_scenes("quad_tiny64")
    r32, r64 = ro.set_rays("quad_tiny"), ro.set_rays("quad_tiny64")
    out = np.full(len(r32) + 1, 0x5a5a5a5a, np.uint32)
    vp = ctypes.c_void_p
    assert L.ceres_ray_order_cpu(f64._h, r32.ctypes.data_as(vp), len(r32), out.ctypes.data_as(vp)) == -6
    assert L.ceres_ray_order_cpu_f64(f32._h, r64.ctypes.data_as(vp), len(r64), out.ctypes.data_as(vp)) == -6
    assert L.ceres_ray_order_cpu(None, r32.ctypes.data_as(vp), len(r32), out.ctypes.data_as(vp)) == -1
    assert L.ceres_ray_order_cpu(f32._h, None, len(r32), out.ctypes.data_as(vp)) == -1
    assert L.ceres_ray_order_cpu(f32._h, r32.ctypes.data_as(vp), len(r32), None) == -1
    assert L.ceres_ray_order_cpu(f32._h, r32.ctypes.data_as(vp), 1 << 31, out.ctypes.data_as(vp)) == -6
    assert (out == 0x5a5a5a5a).all()
    assert L.ceres_ray_order_cpu(f32._h, None, 0, None) == 0          # nothing to order


def test_coherence_floor(pkg):
    """A floor against a key that does nothing: on the shuffled camera rays of the dragon 333 x 217 view nearly
    every group of 64 holds a hit ray; in the order at most half as many do."""
    rays, mesh, bvh = ro.dragon_view_rays()
    cpu = pkg.CpuScene(mesh, bvh)
    try:
        hits, _, _ = cpu.trace(rays)
        order = cpu.ray_order(rays)
    finally:
        cpu.close()
    hit = hits["prim"] >= 0
    share = float(hit.mean())
    h_shuffled, groups = ro.hit_groups(hit, np.arange(len(rays)))
    h_ordered, _ = ro.hit_groups(hit, order)
    print("hit share %.3f, groups %d, hit-bearing: shuffled %d, ordered %d" % (share, groups, h_shuffled, h_ordered))
    assert share < 0.3 and h_shuffled >= 0.9 * groups                 # the input's own conditions
    assert h_ordered <= h_shuffled / 2


def test_scratch_bytes_is_host_arithmetic(pkg):
    """ceres_ray_order_scratch_bytes touches no device and does not decrease as n grows."""
    sizes = [pkg.ray_order_scratch_bytes(n) for n in (0, 1, 63, 64, 65, 4099, 1 << 20, (1 << 31) - 1)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[-1] >= 12 * ((1 << 31) - 1)
