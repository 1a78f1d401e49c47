"""Shaded ray queries on double scenes, GPU path (ceres_shade_rays_f64 / ceres_shade_rays_f64_device,
Scene.shade / shade_device on a double scene, `./render --double --rays ... --pixels-out`):
render<double>()'s pixel for caller-supplied ray64 records.

The same pins as tests/test_shade_cpu_f64.py -- fed a fixture's primary rays, the query must return the
reference's recorded double pixels, Scene.render's framebuffer and the reference's PPM, in both
arithmetics -- plus GPU-against-CPU equality on rays no camera makes, tails with guard regions around
all four outputs, the device call on two streams, refusals, a stats scene, the render call's bytes
after a batch of shade calls, a non-finite sun and the CLI.  No tolerance anywhere."""
import ctypes
import subprocess

import numpy as np
import pytest

import shade64_common as s64
import trace64_common as t64

pytestmark = pytest.mark.gpu

ALL = s64.ALL


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def scenes(gpu):
    """Scenes created once per module: get(name, build, stats) -> Scene, cpu(name, build) -> CpuScene."""
    cache = {}

    class Get:
        def __call__(self, name, build="exact", stats=False):
            key = (name, build, stats)
            if key not in cache:
                _, mesh, bvh, _, _, _, _ = t64.fixture(name, build)
                cache[key] = gpu.Scene(mesh, bvh, stats=stats)
            return cache[key]

        def cpu(self, name, build="exact"):
            key = (name, build, "cpu")
            if key not in cache:
                _, mesh, bvh, _, _, _, _ = t64.fixture(name, build)
                cache[key] = gpu.CpuScene(mesh, bvh)
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


def shader(scene):
    return lambda rays, sun, mode, **out: scene.shade(rays, sun, mode=mode, **out)


def renderer(scene):
    return lambda basis, sun, W, H, mode: scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


@pytest.mark.parametrize("build", s64.BUILDS)
@pytest.mark.parametrize("name", s64.FRAME_FIXTURES)
def test_camera_rays_give_the_reference_frame(gpu, scenes, name, build):
    """tri1 (the root is a leaf), quad (one step, no stack), degenerate, proc_101, bunny_1x1 (one ray: 63
    idle lanes), dragon_333x217 (all-miss, all-hit and mixed wavefronts, a tail of 5): the reference's
    recorded pixels, Scene.render's framebuffer and the PPM, bit for bit."""
    if build == "exact":
        s64.check_camera_rays(gpu, name)
    elif name in t64.REF_FIXTURES:
        s64.check_camera_rays_fma(gpu, name)
    sc = scenes(name, build)
    s64.check_frame_against_fixture(gpu, shader(sc), renderer(sc), tracer(sc), name, build)


@pytest.mark.parametrize("label", s64.COMPOSITION_SETS)
def test_shade_equals_the_composition_of_the_ray_queries(gpu, label):
    mesh, bvh, _, _ = s64.ray_set(label)
    sc = gpu.Scene(mesh, bvh)
    try:
        s64.check_composition(gpu, shader(sc), tracer(sc), label)
    finally:
        sc.close()


@pytest.mark.parametrize("build", s64.BUILDS)
@pytest.mark.parametrize("label", s64.PARITY_SETS)
def test_gpu_equals_cpu(gpu, label, build):
    """Pixels (NaNs canonical, positions equal), rgb8, hits and status byte for byte against the CPU path,
    and the counters, on the adversarial set, both smallest trees, the lattice and the brute-force set.
    A pixel mismatch that traces to pow24_from_double against the host's std::pow is a finding."""
    mesh, bvh, rays, sun = s64.ray_set(label, build)
    mode = s64.mode_of(gpu, build)
    sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
    try:
        c = cpu.shade(rays, sun, mode=mode, **ALL)
        s64.check_parity_set_input(label, build, c[3])
        g = sc.shade(rays, sun, mode=mode, **ALL)
        bad = np.flatnonzero((g[0].view(np.uint64) != c[0].view(np.uint64)).any(axis=1) & ~np.isnan(c[0]).any(axis=1))
        assert len(bad) == 0, (label, build, bad[:4], g[0][bad[:4]].view(np.uint64), c[0][bad[:4]].view(np.uint64))
        assert s64.outputs_equal(g[:4], c[:4]), (label, build)
        for k in ("rays", "hits", "primary_rays", "shadow_rays"):
            assert g[4][k] == c[4][k], (label, build, k)
    finally:
        sc.close()
        cpu.close()


def guarded(torch, n, width, dtype, fill):
    """n records of `width` elements with 64 records of guard in front and behind."""
    return torch.full(((n + 128) * width,), fill, dtype=dtype, device="cuda")


def test_tails_and_guard_regions(gpu, scenes):
    """n_rays that does not fill the last wavefront, and every "only one output" combination: the first n
    results of the full run, the guard records in front of and behind each buffer untouched (the 24-B
    and 3-B records make an over-wide store easy to write)."""
    import torch
    rays, sun = t64.adversarial_rays(), t64.fixture(t64.DRAGON)[4]
    sc = scenes(t64.DRAGON)
    full = sc.shade(rays, sun, **ALL)
    assert set(np.unique(full[3][:63]).tolist()) >= {0, 1} and (full[3][:4097] == 2).any()
    ref = [full[0], full[1], full[2].view(np.int64).reshape(-1, 4), full[3]]
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    spec = [(3, torch.float64, 7.5), (3, torch.uint8, 0xa5), (4, torch.int64, 0x5a5a5a5a5a5a5a5a), (1, torch.uint8, 0xa5)]
    for n in (1, 63, 64, 65, 4097):
        for want in [(True,) * 4] + [tuple(k == q for q in range(4)) for k in range(4)]:
            bufs = [guarded(torch, n, w, dt, fill) for w, dt, fill in spec]
            ptr = [b[64 * w:].data_ptr() if on else 0 for b, (w, _, _), on in zip(bufs, spec, want)]
            d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
            sc.shade_device(d_rays.data_ptr(), n, sun, d_pixels=ptr[0], d_rgb8=ptr[1], d_hits16=ptr[2], d_status=ptr[3],
                            d_counters=d_cnt.data_ptr(), stream=st)
            torch.cuda.synchronize()
            for k, (b, (w, _, fill), on) in enumerate(zip(bufs, spec, want)):
                a = b.cpu().numpy()
                guard = np.concatenate([a[:64 * w], a[(64 + n) * w:]])
                assert (guard == a.dtype.type(fill)).all(), (n, want, s64.OUTPUTS[k])
                body = a[64 * w:(64 + n) * w]
                if on:
                    exp = ref[k][:n]
                    assert (s64.pixel_bytes(body) == s64.pixel_bytes(exp)) if k == 0 else (body.tobytes() == exp.tobytes()), \
                        (n, want, s64.OUTPUTS[k])
                else:
                    assert (body == a.dtype.type(fill)).all(), (n, want, s64.OUTPUTS[k])
            c = d_cnt.cpu().numpy()
            n_hit, n_blocked = int((full[3][:n] != 0).sum()), int((full[3][:n] == 2).sum())
            assert (c[0], c[1], c[2], c[3]) == (n + n_hit, n_hit + n_blocked, n, n_hit) and not c[4:].any(), (n, want)


def test_device_call_on_two_streams(gpu, scenes):
    """Two shade_device calls of one scene on two streams (one part of the rays each), one synchronise:
    the host call's results; each part's own counters."""
    import torch
    rays, sun = t64.adversarial_rays(), t64.fixture(t64.DRAGON)[4]
    sc = scenes(t64.DRAGON)
    full = sc.shade(rays, sun, **ALL)
    n, cut = len(rays), 2048
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_px = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros((n, 3), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    sc.shade_device(d_rays.data_ptr(), cut, sun, d_pixels=d_px.data_ptr(), d_rgb8=d_rgb.data_ptr(), d_hits16=d_hits.data_ptr(),
                    d_status=d_st.data_ptr(), d_counters=d_cnt[0].data_ptr(), stream=s0.cuda_stream)
    sc.shade_device(d_rays[cut:].data_ptr(), n - cut, sun, d_pixels=d_px[cut:].data_ptr(), d_rgb8=d_rgb[cut:].data_ptr(),
                    d_hits16=d_hits[cut:].data_ptr(), d_status=d_st[cut:].data_ptr(), d_counters=d_cnt[1].data_ptr(),
                    stream=s1.cuda_stream)
    torch.cuda.synchronize()
    got = (d_px.cpu().numpy(), d_rgb.cpu().numpy(), d_hits.cpu().numpy().view(gpu.HIT64_DTYPE).reshape(-1), d_st.cpu().numpy())
    assert s64.outputs_equal(got, full[:4])
    c = d_cnt.cpu().numpy()
    for k, part in enumerate((full[3][:cut], full[3][cut:])):
        n_hit, n_blocked = int((part != 0).sum()), int((part == 2).sum())
        assert (c[k, 0], c[k, 1], c[k, 2], c[k, 3]) == (len(part) + n_hit, n_hit + n_blocked, len(part), n_hit)
        assert not c[k, 4:].any()


def test_refusals_write_nothing(gpu, scenes):
    """A misaligned rays / hits / pixels pointer, a bad mode, no output, n >= 2^31 and a float scene are
    refused before any launch: outputs and counters keep their bytes."""
    import torch
    rays, sun = t64.adversarial_rays(), np.asarray(t64.fixture(t64.DRAGON)[4], np.float64)
    sc = scenes(t64.DRAGON)
    n = 64
    d_rays = torch.from_numpy(np.array(rays[:n + 1])).cuda()
    d_px = torch.full((3 * n + 4,), 7.5, dtype=torch.float64, device="cuda")
    d_hits = torch.full((4 * n + 4,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xa5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((8,), 77, dtype=torch.int64, device="cuda")
    L = gpu.lib()
    dp = sun.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(h, r, count, mode, px, hits, status, s=dp):
        return L.ceres_shade_rays_f64_device(h, r, count, s, mode, px, None, hits, status, d_cnt.data_ptr(), None)

    r, px, hits, status = d_rays.data_ptr(), d_px.data_ptr(), d_hits.data_ptr(), d_st.data_ptr()
    assert call(sc._h, r + 8, n, 0, px, hits, status) == -1           # rays not 16-byte aligned
    assert call(sc._h, r, n, 0, px, hits + 8, status) == -1           # hits not 16-byte aligned
    assert call(sc._h, r, n, 0, px + 4, hits, status) == -1           # pixels not 8-byte aligned
    assert call(sc._h, r, n, gpu.MODE_PRIMARY, px, hits, status) == -1
    assert call(sc._h, r, n, gpu.MODE_QBVH4, px, hits, status) == -1
    assert call(sc._h, r, n, gpu.MODE_ROBUST, px, hits, status) == -6  # float-only
    assert call(sc._h, r, n, 0, None, None, None) == -1               # no output asked for
    assert call(sc._h, None, n, 0, px, hits, status) == -1 and call(sc._h, r, n, 0, px, hits, status, s=None) == -1
    assert call(sc._h, r, 1 << 31, 0, px, hits, status) == -6
    mesh, bvh, _ = gpu.prepare(gpu.configs.CONFIGS["tri1"])
    f = gpu.Scene(mesh, bvh)
    try:
        assert call(f._h, r, n, 0, px, hits, status) == -6            # a float scene
    finally:
        f.close()
    assert call(sc._h, r, 0, 0, px, hits, status) == 0                # n = 0: a successful no-op
    torch.cuda.synchronize()
    assert (d_px.cpu().numpy() == 7.5).all() and (d_hits.cpu().numpy() == 0x5a5a5a5a5a5a5a5a).all()
    assert (d_st.cpu().numpy() == 0xa5).all() and (d_cnt.cpu().numpy() == 77).all()
    assert call(sc._h, r, n, 0, px + 8, hits, status) == 0            # 8-byte aligned pixels are enough
    torch.cuda.synchronize()
    exp = sc.shade(rays[:n], sun)[0]
    assert s64.pixel_bytes(d_px.cpu().numpy()[1:3 * n + 1]) == s64.pixel_bytes(exp)
    with pytest.raises(gpu.CeresError, match="error -1"):
        sc.shade(rays[:4], sun, pixels=False)
    p0, q0, h0, s0, st = sc.shade(np.zeros((0, 8), np.float64), sun, **ALL)
    assert p0.shape == (0, 3) and p0.dtype == np.float64 and q0.shape == (0, 3) and len(h0) == 0 and len(s0) == 0
    assert st["rays"] == 0
    for sym in ("ceres_shade_rays_f64", "ceres_shade_rays_f64_device", "ceres_shade_rays_cpu_f64", "ceres_camera_rays_f64"):
        assert sym in gpu.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "ceres_shade_rays64_k" in L.ceres_kernel_names().decode().split(",")


def test_stats_scene_runs_the_same_kernels(gpu, scenes):
    rays, sun = t64.adversarial_rays(), t64.fixture(t64.DRAGON)[4]
    a = scenes(t64.DRAGON).shade(rays, sun, **ALL)
    b = scenes(t64.DRAGON, stats=True).shade(rays, sun, **ALL)
    assert s64.outputs_equal(a[:4], b[:4])
    assert (b[4]["rays"], b[4]["hits"]) == (a[4]["rays"], a[4]["hits"])
    assert b[4]["node_pairs"] == 0 and b[4]["tri_tests"] == 0


def test_render_is_undisturbed_by_shade_calls(gpu):
    """Scene.render's bytes and counters before and after a batch of shade calls are identical."""
    rays = t64.adversarial_rays()
    for build in s64.BUILDS:
        cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(t64.DRAGON, build)
        sc = gpu.Scene(mesh, bvh)
        try:
            W, H = cfg["W"], cfg["H"]
            mode = s64.mode_of(gpu, build)
            px0, rgb0, st0 = sc.render(basis, sun, W, H, mode=mode)
            sc.shade(rays, sun, mode=mode, **ALL)
            sc.shade(gpu.camera_rays64(basis, W, H, arith=s64.arith_of(build)), sun, mode=mode)
            px1, rgb1, st1 = sc.render(basis, sun, W, H, mode=mode)
            assert px0.tobytes() == px1.tobytes() and rgb0.tobytes() == rgb1.tobytes()
            for k in ("rays", "hits", "primary_rays", "shadow_rays", "node_pairs", "tri_tests"):
                assert st0[k] == st1[k], k
        finally:
            sc.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_non_finite_sun(gpu, scenes, bad):
    """65 of the dragon's camera rays (a wavefront and a tail of one: 40 that hit, 25 others) under a sun
    with a NaN or an infinite coordinate: status and NaN positions equal the CPU path's."""
    cfg, _, _, basis, sun, _, rec = t64.fixture(t64.DRAGON)
    all_rays = gpu.camera_rays64(basis, cfg["W"], cfg["H"])
    hit_px = rec["pixel"][rec["prim"] >= 0].astype(np.int64)
    rays = np.ascontiguousarray(np.concatenate([all_rays[hit_px[:40]], all_rays[:25]]))
    assert len(rays) == 65
    s = np.array(sun, np.float64)
    s[1] = bad
    c = scenes.cpu(t64.DRAGON).shade(rays, s, **ALL)
    g = scenes(t64.DRAGON).shade(rays, s, **ALL)
    assert (c[3] != 0).sum() >= 40
    assert np.array_equal(g[3], c[3]) and np.array_equal(np.isnan(g[0]), np.isnan(c[0]))
    assert s64.outputs_equal(g[:4], c[:4])


def test_cli(gpu, scenes, tmp_path):
    """./render --double --rays ... --sun ... --pixels-out ... on the dragon's camera rays reproduces the
    Python bytes, on the GPU and with --cpu; --double --hits-out alone still writes what it wrote; a
    file that is not a whole number of ray64 records is bad usage."""
    cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(t64.DRAGON)
    rays = gpu.camera_rays64(basis, cfg["W"], cfg["H"])
    exp = scenes(t64.DRAGON).shade(rays, sun, **ALL)
    old_hits, old_occ, _ = scenes(t64.DRAGON).trace(rays, closest=True, occluded=True)
    assert t64.hits_equal(old_hits, exp[2])
    rf = tmp_path / "rays.bin"
    rf.write_bytes(rays.tobytes())
    obj = gpu.configs.obj_path(cfg)
    base = [gpu.CLI_PATH, obj, "--exact", "--double", "--rays", str(rf)]
    if cfg.get("rotate"):
        base += ["--rotate", str(cfg["rotate"][0]), repr(float(cfg["rotate"][1]))]
    sun_args = ["--sun"] + [repr(float(x)) for x in np.asarray(sun, np.float64)]
    for extra in ([], ["--cpu"]):
        out = {k: tmp_path / (k + ("_cpu" if extra else "") + ".bin") for k in s64.OUTPUTS}
        r = subprocess.run(base + sun_args + ["--pixels-out", str(out["pixels"]), "--rgb8-out", str(out["rgb8"]), "--hits-out",
                                              str(out["hits"]), "--status-out", str(out["status"]), "--json"] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert out["pixels"].read_bytes() == exp[0].tobytes(), extra
        assert out["rgb8"].read_bytes() == exp[1].tobytes(), extra
        assert out["hits"].read_bytes() == exp[2].tobytes(), extra
        assert out["status"].read_bytes() == exp[3].tobytes(), extra
        assert '"shadow_rays": %d' % int((exp[3] != 0).sum()) in r.stdout
        h, o = tmp_path / ("h%d.bin" % len(extra)), tmp_path / ("o%d.bin" % len(extra))
        r = subprocess.run(base + ["--hits-out", str(h), "--occluded-out", str(o)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert h.read_bytes() == old_hits.tobytes() and o.read_bytes() == old_occ.tobytes(), extra
    short = tmp_path / "short.bin"
    short.write_bytes(rays.tobytes()[:-32])
    r = subprocess.run(base[:4] + ["--rays", str(short)] + sun_args + ["--pixels-out", str(tmp_path / "x.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--double" in r.stderr and not (tmp_path / "x.bin").exists()
