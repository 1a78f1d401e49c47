"""Shaded ray queries on the CPU path (ceres_shade_rays_cpu, CpuScene.shade) and the host ray generator
(ceres_camera_rays): render()'s pixel for caller-supplied rays.

The oracle is the reference's own frame: fed the primary rays of a fixture's view, a shaded ray query
must return CpuScene.render's float framebuffer bit for bit and the reference's PPM byte for byte, in
the contraction-free build and in the reference CMake build's arithmetic.  For rays no camera makes,
the query must equal the composition a caller would otherwise write from the ray queries.  No GPU
needed; no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import shade_common as sh
import trace_common as tc


@pytest.fixture(scope="module")
def cpu_scene(pkg):
    cache = {}

    def get(name, arith=0):
        if (name, arith) not in cache:
            _, mesh, bvh, _, _, _, _ = tc.fixture(name, arith)
            cache[name, arith] = pkg.CpuScene(mesh, bvh)
        return cache[name, arith]

    yield get
    for s in cache.values():
        s.close()


def shader(scene, **kw):
    return lambda rays, sun, mode, **out: scene.shade(rays, sun, mode=mode, **out, **kw)


def renderer(scene):
    return lambda basis, sun, W, H, mode: scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


@pytest.mark.parametrize("name", sh.shaded_fixtures())
def test_exact_build_equals_the_reference_frame(pkg, cpu_scene, name):
    sc = cpu_scene(name)
    sh.check_frame_against_fixture(pkg, shader(sc), renderer(sc), tracer(sc), name, pkg.ARITH_EXACT)


@pytest.mark.parametrize("name", sh.shaded_fixtures())
def test_fma_build_equals_the_reference_frame(pkg, cpu_scene, name):
    sc = cpu_scene(name, pkg.ARITH_FMA)
    sh.check_frame_against_fixture(pkg, shader(sc), renderer(sc), tracer(sc), name, pkg.ARITH_FMA)


def test_stats_are_the_sum_of_both_walks(pkg, cpu_scene):
    """node_pairs / tri_tests as ceres_render_cpu_f32 counts them, on the dragon's view."""
    cfg, _, _, basis, sun, _, _ = tc.fixture(tc.DRAGON)
    sc = cpu_scene(tc.DRAGON)
    _, _, rst = sc.render(basis, sun, cfg["W"], cfg["H"], want_rgb8=False)
    st = sc.shade(pkg.camera_rays(basis, cfg["W"], cfg["H"]), sun)[4]
    assert (st["node_pairs"], st["tri_tests"]) == (rst["node_pairs"], rst["tri_tests"])
    assert st["node_pairs"] > 0 and st["tri_tests"] > 0


@pytest.mark.parametrize("name", ["dragon_333x217", "bunny_1x1"])
def test_ray_generator_equals_the_numpy_rays(pkg, name):
    cfg, _, _, basis, _, _, _ = tc.fixture(name)
    W, H = cfg["W"], cfg["H"]
    a = pkg.camera_rays(basis, W, H)
    b = pkg.camera_rays_native(basis, W, H, pkg.ARITH_EXACT)
    assert a.shape == b.shape == (W * H, 8) and a.tobytes() == b.tobytes()
    c = pkg.camera_rays(basis, W, H, arith=pkg.ARITH_FMA)
    assert c.tobytes() == pkg.camera_rays_native(basis, W, H, pkg.ARITH_FMA).tobytes()
    assert np.array_equal(c[:, [0, 1, 2, 6, 7]], a[:, [0, 1, 2, 6, 7]])
    if W * H > 1:
        assert c.tobytes() != a.tobytes()                             # contraction changes some direction bits


@pytest.mark.parametrize("k", range(3))
def test_shade_equals_the_composition_of_the_ray_queries(pkg, cpu_scene, k):
    name, rays, sun = sh.composition_sets()[k]
    assert np.isfinite(sun).all()
    sc = cpu_scene(name)
    mesh = tc.fixture(name)[1]
    _, _, _, status = sh.check_composition(pkg, mesh, shader(sc), tracer(sc), rays, sun)
    assert set(np.unique(status).tolist()) == {0, 1, 2}, (name, np.bincount(status, minlength=3))


@pytest.mark.parametrize("label", sh.PARITY_SETS)
def test_gpu_parity_sets_meet_their_floors(pkg, label):
    """The ray sets and suns of the GPU-against-CPU comparison (test_gpu_shade.py), on the CPU path in
    the four modes: lit hits in every set, at least 50 rays of each status on the dragon and proc300 sets."""
    for mode, arith in tc.modes(pkg):
        mesh, bvh, rays, sun = sh.parity_set(label, arith)
        sc = pkg.CpuScene(mesh, bvh)
        try:
            sh.check_parity_set_input(label, sc.shade(rays, sun, mode=mode, pixels=False, status=True)[3])
        finally:
            sc.close()


def test_threads_and_single_outputs(pkg, cpu_scene):
    sc = cpu_scene(tc.DRAGON)
    rays, sun = tc.adversarial_rays(), tc.fixture(tc.DRAGON)[4]
    full = sc.shade(rays, sun, pixels=True, rgb8=True, hits=True, status=True, threads=1)
    again = sc.shade(rays, sun, pixels=True, rgb8=True, hits=True, status=True, threads=8)
    assert sh.outputs_equal(full[:4], again[:4]) and full[4]["hits"] == again[4]["hits"]
    for k, key in enumerate(("pixels", "rgb8", "hits", "status")):
        only = sc.shade(rays, sun, **{q: q == key for q in ("pixels", "rgb8", "hits", "status")})
        assert [o is not None for o in only[:4]] == [q == k for q in range(4)]
        assert only[k].tobytes() == full[k].tobytes(), key


def test_refusals_leave_the_outputs_alone(pkg, cpu_scene):
    L = pkg.lib()
    sc = cpu_scene(tc.DRAGON)
    rays = np.array(tc.adversarial_rays()[:4])
    sun = np.asarray(tc.fixture(tc.DRAGON)[4], np.float32)
    px = np.full((4, 3), 7.5, np.float32)
    rgb = np.full((4, 3), 0xa5, np.uint8)
    hits = np.full(4, 0x5a, np.uint8).repeat(16).view(pkg.HIT_DTYPE)
    status = np.full(4, 0xa5, np.uint8)
    before = [a.tobytes() for a in (px, rgb, hits, status)]
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    fp = sun.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    call = lambda h, n, mode, outs=True: L.ceres_shade_rays_cpu(     # noqa: E731
        h, vp(rays), n, fp, mode, *((vp(px), vp(rgb), vp(hits), vp(status)) if outs else (None, None, None, None)), None, 0)
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"], f64=True)
    d = pkg.CpuScene(mesh, bvh)
    try:
        assert call(d._h, 4, 0) == -6                                 # a double scene
    finally:
        d.close()
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY):
        assert call(sc._h, 4, bad) == -1
    assert call(sc._h, 4, 0, outs=False) == -1                        # no output asked for
    assert call(sc._h, 1 << 31, 0) == -6
    assert call(sc._h, 0, 0) == 0                                     # a successful no-op
    assert [a.tobytes() for a in (px, rgb, hits, status)] == before
    with pytest.raises(pkg.CeresError, match="error -1"):
        sc.shade(rays, sun, pixels=False)
    p0, q0, h0, s0, st = sc.shade(np.zeros((0, 8), np.float32), sun, pixels=True, rgb8=True, hits=True, status=True)
    assert p0.shape == (0, 3) and q0.shape == (0, 3) and len(h0) == 0 and len(s0) == 0 and st["rays"] == 0
    for sym in ("ceres_shade_rays", "ceres_shade_rays_device", "ceres_shade_rays_cpu", "ceres_camera_rays"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "ceres_shade_rays_k" in L.ceres_kernel_names().decode().split(",")
