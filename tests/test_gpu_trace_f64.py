"""Ray queries on double-precision scenes, GPU (ceres_trace_rays_f64 / ceres_trace_rays_f64_device,
Scene.trace / trace_device on a double scene; the kernel ceres_trace_rays64_k of render64.hip): the pins
of tests/test_trace_cpu_f64.py -- the reference's render<double> records through rebuilt rays, bit for
bit, in both arithmetics, the brute force over all triangles, and the reference's own answers to the
stored caller rays of tests/golden/rays64/ -- plus GPU against CPU byte for byte
on adversarial rays (non-finite ones included), tails with guard regions, the device call on two
streams, and the render call's bytes after trace calls."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import trace64_common as t64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


def _scene_arrays(name, build):
    if name in t64.BRUTE_SCENES and name != "quad":
        return t64.brute_scene(name)
    return t64.fixture(name, build)[1:3]


@pytest.fixture(scope="module")
def scenes(gpu):
    """Scenes created once per module: get(name, build, stats) -> Scene, cpu(name, build) -> CpuScene."""
    cache = {}

    class Get:
        def __call__(self, name, build="exact", stats=False):
            key = (name, build, stats)
            if key not in cache:
                cache[key] = gpu.Scene(*_scene_arrays(name, build), stats=stats)
            return cache[key]

        def cpu(self, name, build="exact"):
            key = (name, build, "cpu")
            if key not in cache:
                cache[key] = gpu.CpuScene(*_scene_arrays(name, build))
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


@pytest.mark.parametrize("name", t64.EXACT_FIXTURES)
def test_closest_hit_equals_reference_double_records(gpu, scenes, name):
    """A stats scene: node_pairs / tri_tests are the reference's Statistics; a plain scene: the same hits."""
    _, hits = t64.check_closest_against_fixture(gpu, tracer(scenes(name, stats=True)), name)
    _, hits2 = t64.check_closest_against_fixture(gpu, tracer(scenes(name)), name, check_stats=False)
    assert t64.hits_equal(hits, hits2)


@pytest.mark.parametrize("name", t64.OCCLUSION_FIXTURES)
def test_occlusion_equals_reference_shadow_flags(gpu, scenes, name):
    t64.check_occlusion_against_fixture(gpu, tracer(scenes(name, stats=True)), name)
    t64.check_occlusion_against_fixture(gpu, tracer(scenes(name)), name)


@pytest.mark.parametrize("name", t64.REF_FIXTURES)
def test_closest_hit_equals_reference_cmake_build_records(gpu, scenes, name):
    """CERES_MODE_FMA on an ARITH_FMA scene, rays rebuilt with a correctly rounded fma."""
    t64.check_closest_against_fixture(gpu, tracer(scenes(name, "ref", stats=True)), name, build="ref")
    t64.check_closest_against_fixture(gpu, tracer(scenes(name, "ref")), name, build="ref", check_stats=False)


@pytest.mark.parametrize("which", t64.BRUTE_SCENES)
def test_closest_hit_equals_brute_force(gpu, scenes, which):
    t64.check_against_brute_force(gpu, tracer(scenes(which)), which)
    t64.check_against_brute_force(gpu, tracer(scenes(which, stats=True)), which)


@pytest.fixture(scope="module")
def ray_scenes(gpu):
    """get(set, build, stats) -> the Scene of a double ray set's scene (tests/golden/rays64/<set>.npz), created once."""
    cache = {}

    def get(name, build="exact", stats=False):
        key = (t64.ray_set_config(name)["obj"], build, stats)
        if key not in cache:
            cache[key] = gpu.Scene(*t64.ray_set_scene(name, build), stats=stats)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("variant", t64.RAY_VARIANTS64)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_caller_rays_equal_the_reference_traverser(gpu, ray_scenes, name, variant):
    """Every stored double ray, the non-finite ones included, against the reference's own
    traverse(ray, intersector) in its double builds: a production scene with both queries, closest
    only and occluded only; a stats scene in stored order, and split into the rays without and with
    a NaN for the Statistics.  lattice_ties64: exact ties in u, v, w, t = tmin, t = tmax and
    coincident triangles through dev64::trace's fmin / fmax slabs."""
    build = t64.variant_mode(gpu, variant)[1]
    prod, st = tracer(ray_scenes(name, build)), tracer(ray_scenes(name, build, stats=True))
    t64.check_against_ray_fixture64(gpu, prod, name, variant, stats=False)
    t64.check_against_ray_fixture64(gpu, prod, name, variant, stats=False, occluded=False)
    t64.check_against_ray_fixture64(gpu, prod, name, variant, stats=False, closest=False)
    t64.check_against_ray_fixture64(gpu, st, name, variant, stats=False)
    t64.check_against_ray_fixture64(gpu, st, name, variant, stats=True)


def test_gpu_equals_cpu_on_adversarial_rays(gpu, scenes):
    """Both arithmetics, plain and stats scenes: hit bytes and occlusion bytes identical, NaN / +-inf
    origins and directions and the zero direction included; once in stored order, once reversed
    without the last 13 rays (another tail wave); a stats scene's counters equal the CPU path's."""
    rays = t64.adversarial_rays()
    orders = [np.array(rays), np.ascontiguousarray(rays[::-1][:-13])]
    assert len(orders[0]) % 64 != len(orders[1]) % 64 and len(orders[1]) % 64 != 0
    for mode, build in t64.modes(gpu):
        for r in orders:
            hc, oc, sc = scenes.cpu(t64.DRAGON, build).trace(r, mode=mode, closest=True, occluded=True)
            t64.check_adversarial_input(r, hc)
            for stats in (False, True):
                hg, og, st = scenes(t64.DRAGON, build, stats).trace(r, mode=mode, closest=True, occluded=True)
                assert t64.hits_equal(hg, hc), (mode, stats)
                assert np.array_equal(og, oc), (mode, stats)
                assert st["rays"] == len(r) and st["hits"] == int((hc["prim"] >= 0).sum())
                if stats:
                    assert (st["node_pairs"], st["tri_tests"]) == (sc["node_pairs"], sc["tri_tests"]), mode
            ho, _, _ = scenes(t64.DRAGON, build).trace(r, mode=mode, closest=True, occluded=False)
            _, oo, so = scenes(t64.DRAGON, build).trace(r, mode=mode, closest=False, occluded=True)
            assert t64.hits_equal(ho, hc) and np.array_equal(oo, oc) and so["hits"] == int(oc.sum())


@pytest.mark.parametrize("name", t64.TINY_FIXTURES)
def test_gpu_equals_cpu_on_the_smallest_trees(gpu, scenes, name):
    """tri1 (the root is a leaf) and quad (a root with two leaf children): 357 rays, five waves and a
    tail of 37, both arithmetics, plain and stats scenes."""
    rays = t64.tiny_tree_rays(name)
    assert len(rays) == 5 * 64 + 37
    open_rays = np.array(rays)
    open_rays[:, 6:8] = (0, t64.DBL_MAX)
    for mode, build in t64.modes(gpu):
        cpu = scenes.cpu(name, build)
        hc, oc, sc = cpu.trace(rays, mode=mode, closest=True, occluded=True)
        t64.check_tiny_tree_input(name, hc, cpu.trace(open_rays, mode=mode, closest=True)[0])
        for stats in (False, True):
            hg, og, st = scenes(name, build, stats).trace(rays, mode=mode, closest=True, occluded=True)
            assert t64.hits_equal(hg, hc), (mode, stats)
            assert np.array_equal(og, oc), (mode, stats)
            assert st["rays"] == len(rays) and st["hits"] == int((hc["prim"] >= 0).sum())
            if stats:                                                 # tri1: tests and no steps
                assert (st["node_pairs"], st["tri_tests"]) == (sc["node_pairs"], sc["tri_tests"]), mode
                assert (st["node_pairs"] == 0) == (name == "tri1") and st["tri_tests"] > 0


def test_tails_and_guard_regions(gpu, scenes):
    """n_rays that does not fill the last wavefront: the first n results of the full run, and the 64
    records behind each output buffer untouched; idle lanes count nothing."""
    import torch
    rays = t64.adversarial_rays()
    sc = scenes(t64.DRAGON, stats=True)
    cpu = scenes.cpu(t64.DRAGON)
    full_h, full_o, _ = sc.trace(rays, closest=True, occluded=True)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n in (1, 63, 64, 65, 4097):
        d_hits = torch.full((n + 64, 4), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
        d_occ = torch.full((n + 64,), 0xa5, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        sc.trace_device(d_rays.data_ptr(), n, d_hits16=d_hits.data_ptr(), d_occluded=d_occ.data_ptr(),
                        d_counters=d_cnt.data_ptr(), stream=st)
        torch.cuda.synchronize()
        h, o, c = d_hits.cpu().numpy(), d_occ.cpu().numpy(), d_cnt.cpu().numpy()
        assert h[:n].tobytes() == full_h[:n].tobytes(), n
        assert np.array_equal(o[:n], full_o[:n]), n
        assert (h[n:] == 0x5a5a5a5a5a5a5a5a).all() and (o[n:] == 0xa5).all(), n
        ref = cpu.trace(rays[:n], closest=True)[2]
        assert c[0] == n and c[2] == n and c[3] == 0 and c[6] == 0 and c[7] == 0, n
        assert (c[1], c[4], c[5]) == (int((full_h["prim"][:n] >= 0).sum()), ref["node_pairs"], ref["tri_tests"]), n


def test_device_call_on_two_streams(gpu, scenes):
    """Two trace_device calls of one scene on two streams (one half of the rays each), one
    synchronise: the host call's results; each call's own counters."""
    import torch
    rays = t64.adversarial_rays()
    sc = scenes(t64.DRAGON)
    full_h, full_o, _ = sc.trace(rays, closest=True, occluded=True)
    n = len(rays)
    cut = 2048
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    sc.trace_device(d_rays.data_ptr(), cut, d_hits16=d_hits.data_ptr(), d_occluded=d_occ.data_ptr(),
                    d_counters=d_cnt[0].data_ptr(), stream=s0.cuda_stream)
    sc.trace_device(d_rays[cut:].data_ptr(), n - cut, d_hits16=d_hits[cut:].data_ptr(), d_occluded=d_occ[cut:].data_ptr(),
                    d_counters=d_cnt[1].data_ptr(), stream=s1.cuda_stream)
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy().tobytes() == full_h.tobytes()
    assert np.array_equal(d_occ.cpu().numpy(), full_o)
    c = d_cnt.cpu().numpy()
    found = full_h["prim"] >= 0
    assert (c[0, 0], c[0, 1]) == (cut, int(found[:cut].sum()))
    assert (c[1, 0], c[1, 1]) == (n - cut, int(found[cut:].sum()))
    assert c[0, 6] == 0 and c[1, 6] == 0


def test_interface_details(gpu, scenes):
    import torch
    sc = scenes(t64.DRAGON)
    rays = np.array(t64.adversarial_rays()[:4])
    h0, o0, st = sc.trace(np.zeros((0, 8), np.float64), closest=True, occluded=True)
    assert len(h0) == 0 and len(o0) == 0 and st["rays"] == 0
    for bad in (gpu.MODE_PRIMARY, gpu.MODE_QBVH4, gpu.MODE_FMA | gpu.MODE_PRIMARY, 0x80):
        with pytest.raises(gpu.CeresError, match="error -1"):
            sc.trace(rays, mode=bad)
    for robust in (gpu.MODE_ROBUST, gpu.MODE_ROBUST | gpu.MODE_FMA):
        with pytest.raises(gpu.CeresError, match="error -6"):
            sc.trace(rays, mode=robust)
    with pytest.raises(gpu.CeresError, match="error -1"):
        sc.trace(rays, closest=False, occluded=False)
    L = gpu.lib()
    h = np.zeros(4, gpu.HIT64_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    assert L.ceres_trace_rays_f64(sc._h, vp(rays), 1 << 31, 0, vp(h), None, None) == -6
    assert L.ceres_trace_rays(sc._h, vp(rays), 4, 0, vp(h), None, None) == -6                      # float call, double scene
    assert L.ceres_trace_rays_device(sc._h, vp(rays), 4, 0, vp(h), None, None, None) == -6
    mesh, bvh, _ = gpu.prepare(gpu.configs.CONFIGS["tri1"])
    f = gpu.Scene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_f64(f._h, vp(rays), 4, 0, vp(h), None, None) == -6               # double call, float scene
        assert L.ceres_trace_rays_f64_device(f._h, vp(rays), 4, 0, vp(h), None, None, None) == -6
    finally:
        f.close()
    # device call: n = 0 and NULL outputs are judged before any pointer is used; a misaligned pointer is refused
    d_rays = torch.from_numpy(np.zeros((5, 8), np.float64)).cuda()
    d_hits = torch.zeros((5, 4), dtype=torch.int64, device="cuda")
    rp, hp = d_rays.data_ptr(), d_hits.data_ptr()
    assert rp % 16 == 0 and hp % 16 == 0
    assert L.ceres_trace_rays_f64_device(sc._h, rp, 0, 0, hp, None, None, None) == 0
    assert L.ceres_trace_rays_f64_device(sc._h, rp, 4, 0, None, None, None, None) == -1
    assert L.ceres_trace_rays_f64_device(sc._h, rp + 8, 4, 0, hp, None, None, None) == -1
    assert L.ceres_trace_rays_f64_device(sc._h, rp, 4, 0, hp + 8, None, None, None) == -1
    assert L.ceres_trace_rays_f64_device(sc._h, rp, 4, gpu.MODE_ROBUST, hp, None, None, None) == -6
    assert L.ceres_trace_rays_f64_device(sc._h, rp, 1 << 31, 0, hp, None, None, None) == -6
    torch.cuda.synchronize()
    assert not d_hits.cpu().numpy().any()                            # none of the refused calls wrote
    assert "ceres_trace_rays64_k" in L.ceres_kernel_names().decode().split(",")


def test_render_is_undisturbed_by_trace_calls(gpu):
    """After trace calls on a double scene, Scene.render of f64/dragon_333x217 still gives the fixture's
    PPM, in both arithmetics."""
    rays = t64.adversarial_rays()
    for build, mode_fma in (("exact", 0), ("ref", gpu.MODE_FMA)):
        cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(t64.DRAGON, build)
        sc = gpu.Scene(mesh, bvh)
        try:
            W, H = cfg["W"], cfg["H"]
            sc.trace(rays, mode=mode_fma, closest=True, occluded=True)
            _, rgb, st = sc.render(basis, sun, W, H, mode=gpu.MODE_FULL | mode_fma)
            assert hashlib.sha256(gpu.ppm(W, H, rgb)).hexdigest() == meta["ppm_sha256"][build], build
            assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"])
            sc.trace(rays, mode=mode_fma, closest=True, occluded=True)
            _, rgb2, _ = sc.render(basis, sun, W, H, mode=gpu.MODE_FULL | mode_fma)
            assert np.array_equal(rgb, rgb2)
        finally:
            sc.close()


def test_cli_double_rays(gpu, scenes, tmp_path):
    """./render --double --rays on tests/golden/tri1.obj, on the GPU and with --cpu: the files hold the
    API's bytes; a file that is not a whole number of 64-byte records is bad usage (status 2)."""
    name = "tri1"
    cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(name)
    rays = gpu.camera_rays64(basis, cfg["W"], cfg["H"])
    hits, occ, st = scenes(name).trace(rays, closest=True, occluded=True)
    assert st["hits"] > 0
    rf, hf, of = tmp_path / "rays.bin", tmp_path / "hits.bin", tmp_path / "occ.bin"
    rf.write_bytes(rays.tobytes())
    args = [os.path.join(os.path.dirname(__file__), "golden", "tri1.obj")]
    if cfg["rotate"]:
        args += ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    for extra in ([], ["--cpu"]):
        for p in (hf, of):
            p.write_bytes(b"")
        r = subprocess.run([gpu.CLI_PATH] + args + ["--exact", "--double", "--json", "--rays", str(rf), "--hits-out", str(hf),
                                                    "--occluded-out", str(of)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert hf.read_bytes() == hits.tobytes() and of.read_bytes() == occ.tobytes(), extra
        assert '"rays": %d, "hits": %d' % (len(rays), st["hits"]) in r.stdout
    (tmp_path / "short.bin").write_bytes(rays.tobytes()[:-32])
    r = subprocess.run([gpu.CLI_PATH] + args + ["--exact", "--double", "--rays", str(tmp_path / "short.bin"), "--hits-out", str(hf)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "64" in r.stderr
