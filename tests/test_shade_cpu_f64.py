"""Shaded ray queries on double scenes, CPU path (ceres_shade_rays_cpu_f64, CpuScene.shade) and the host
ray generator (ceres_camera_rays_f64): render<double>()'s pixel for caller-supplied ray64 records.

The oracle is the reference's own double frame (tests/golden/f64/): fed the primary rays of a fixture's
view, the query must return the recorded pixels and CpuScene.render's framebuffer bit for bit and the
reference's PPM byte for byte, in the contraction-free build and in the reference CMake build's
arithmetic.  For rays no camera makes it must equal the composition a caller would otherwise write
from the double ray queries.  No GPU needed; no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import shade64_common as s64
import trace64_common as t64


@pytest.fixture(scope="module")
def cpu_scene(pkg):
    cache = {}

    def get(name, build="exact"):
        if (name, build) not in cache:
            _, mesh, bvh, _, _, _, _ = t64.fixture(name, build)
            cache[name, build] = pkg.CpuScene(mesh, bvh)
        return cache[name, build]

    yield get
    for s in cache.values():
        s.close()


def shader(scene, **kw):
    return lambda rays, sun, mode, **out: scene.shade(rays, sun, mode=mode, **out, **kw)


def renderer(scene):
    return lambda basis, sun, W, H, mode: scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


@pytest.mark.parametrize("name", s64.FRAME_FIXTURES)
def test_ray_generator_equals_the_numpy_rays(pkg, name):
    s64.check_camera_rays(pkg, name)


@pytest.mark.parametrize("name", t64.REF_FIXTURES)
def test_fma_ray_generator_equals_the_exact_fma(pkg, name):
    s64.check_camera_rays_fma(pkg, name)


@pytest.mark.parametrize("build", s64.BUILDS)
@pytest.mark.parametrize("name", s64.FRAME_FIXTURES)
def test_camera_rays_give_the_reference_frame(pkg, cpu_scene, name, build):
    sc = cpu_scene(name, build)
    _, st = s64.check_frame_against_fixture(pkg, shader(sc), renderer(sc), tracer(sc), name, build)
    # node_pairs / tri_tests: the sum of both walks, as ceres_render_cpu_f64 counts them
    cfg, _, _, basis, sun, _, _ = t64.fixture(name, build)
    rst = sc.render(basis, sun, cfg["W"], cfg["H"], mode=s64.mode_of(pkg, build), want_rgb8=False)[2]
    assert (st["node_pairs"], st["tri_tests"]) == (rst["node_pairs"], rst["tri_tests"])
    assert st["tri_tests"] > 0 and (st["node_pairs"] > 0) == (name != "tri1")


@pytest.mark.parametrize("label", s64.COMPOSITION_SETS)
def test_shade_equals_the_composition_of_the_ray_queries(pkg, label):
    mesh, bvh, _, _ = s64.ray_set(label)
    sc = pkg.CpuScene(mesh, bvh)
    try:
        s64.check_composition(pkg, shader(sc), tracer(sc), label)
    finally:
        sc.close()


@pytest.mark.parametrize("label", s64.PARITY_SETS)
def test_gpu_parity_sets_meet_their_floors(pkg, label):
    """The ray sets and suns of the GPU-against-CPU comparison (test_gpu_shade_f64.py), on the CPU path in
    both arithmetics: lit hits in every set, at least 50 rays of each status on the floored sets."""
    for build in s64.BUILDS:
        mesh, bvh, rays, sun = s64.ray_set(label, build)
        sc = pkg.CpuScene(mesh, bvh)
        try:
            status = sc.shade(rays, sun, mode=s64.mode_of(pkg, build), pixels=False, status=True)[3]
            s64.check_parity_set_input(label, build, status)
        finally:
            sc.close()


def test_threads_and_single_outputs(pkg, cpu_scene):
    sc = cpu_scene(t64.DRAGON)
    rays, sun = t64.adversarial_rays(), t64.fixture(t64.DRAGON)[4]
    full = sc.shade(rays, sun, threads=1, **s64.ALL)
    again = sc.shade(rays, sun, threads=8, **s64.ALL)
    assert s64.outputs_equal(full[:4], again[:4])
    for k in ("rays", "hits", "primary_rays", "shadow_rays", "node_pairs", "tri_tests"):
        assert full[4][k] == again[4][k], k
    for k, key in enumerate(s64.OUTPUTS):
        only = sc.shade(rays, sun, **{q: q == key for q in s64.OUTPUTS})
        assert [o is not None for o in only[:4]] == [q == k for q in range(4)]
        assert only[k].tobytes() == full[k].tobytes(), key


def test_refusals_leave_the_outputs_alone(pkg, cpu_scene):
    L = pkg.lib()
    sc = cpu_scene(t64.DRAGON)
    rays = np.array(t64.adversarial_rays()[:4])
    sun = np.asarray(t64.fixture(t64.DRAGON)[4], np.float64)
    px = np.full((4, 3), 7.5, np.float64)
    rgb = np.full((4, 3), 0xa5, np.uint8)
    hits = np.full(4, 0x5a, np.uint8).repeat(32).view(pkg.HIT64_DTYPE)
    status = np.full(4, 0xa5, np.uint8)
    before = [a.tobytes() for a in (px, rgb, hits, status)]
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    dp = sun.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda h, n, mode, outs=True, r=rays, s=dp: L.ceres_shade_rays_cpu_f64(     # noqa: E731
        h, None if r is None else vp(r), n, s, mode,
        *((vp(px), vp(rgb), vp(hits), vp(status)) if outs else (None, None, None, None)), None, 0)
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"])
    f = pkg.CpuScene(mesh, bvh)
    try:
        assert call(f._h, 4, 0) == -6                                 # a float scene
    finally:
        f.close()
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY):
        assert call(sc._h, 4, bad) == -1
    assert call(sc._h, 4, pkg.MODE_ROBUST) == -6                      # float-only
    assert call(sc._h, 4, 0, outs=False) == -1                        # no output asked for
    assert call(sc._h, 4, 0, r=None) == -1 and call(sc._h, 4, 0, s=None) == -1
    assert call(sc._h, 1 << 31, 0) == -6
    assert call(sc._h, 0, 0) == 0                                     # a successful no-op
    assert [a.tobytes() for a in (px, rgb, hits, status)] == before
    with pytest.raises(pkg.CeresError, match="error -1"):
        sc.shade(rays, sun, pixels=False)
    p0, q0, h0, s0, st = sc.shade(np.zeros((0, 8), np.float64), sun, **s64.ALL)
    assert p0.shape == (0, 3) and p0.dtype == np.float64 and q0.shape == (0, 3) and len(h0) == 0 and len(s0) == 0
    assert st["rays"] == 0
    for sym in ("ceres_shade_rays_f64", "ceres_shade_rays_f64_device", "ceres_shade_rays_cpu_f64", "ceres_camera_rays_f64"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "ceres_shade_rays64_k" in L.ceres_kernel_names().decode().split(",")
