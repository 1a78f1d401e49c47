"""Ray queries on the GPU (ceres_trace_rays / ceres_trace_rays_device, Scene.trace / trace_device): the
same pins as tests/test_trace_cpu.py -- the reference's per-pixel records through rebuilt rays, bit for
bit -- and the reference's own answers to caller-style rays (tests/golden/rays/), plus GPU-against-CPU
equality on the same rays, the octant-specialised loops against the generic loop, tails with guard
regions, the device call on two streams, and the render calls' bytes after a trace."""
import hashlib

import numpy as np
import pytest

import trace_common as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def scenes(gpu):
    """Scenes created once per module: get(name, arith, stats) -> Scene, cpu(name, arith) -> CpuScene."""
    cache = {}

    class Get:
        def __call__(self, name, arith=0, stats=False):
            key = (name, arith, stats)
            if key not in cache:
                _, mesh, bvh, _, _, _, _ = tc.fixture(name, arith)
                cache[key] = gpu.Scene(mesh, bvh, stats=stats)
            return cache[key]

        def cpu(self, name, arith=0):
            key = (name, arith, "cpu")
            if key not in cache:
                _, mesh, bvh, _, _, _, _ = tc.fixture(name, arith)
                cache[key] = gpu.CpuScene(mesh, bvh)
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


@pytest.mark.parametrize("name", tc.CLOSEST_FIXTURES)
def test_closest_hit_equals_reference_records(gpu, scenes, name):
    """Stats scenes: node_pairs / tri_tests are the reference's Statistics; then the production
    kernels (octant-specialised loops) give the same hits."""
    _, hits = tc.check_closest_against_fixture(gpu, tracer(scenes(name, stats=True)), name)
    _, hits2 = tc.check_closest_against_fixture(gpu, tracer(scenes(name)), name, check_stats=False)
    assert tc.hits_equal(hits, hits2)


@pytest.mark.parametrize("name", tc.OCCLUSION_FIXTURES)
def test_occlusion_equals_reference_shadow_flags(gpu, scenes, name):
    tc.check_occlusion_against_fixture(gpu, tracer(scenes(name, stats=True)), name)
    tc.check_occlusion_against_fixture(gpu, tracer(scenes(name)), name)


def test_gpu_equals_cpu_on_adversarial_rays(gpu, scenes):
    """{exact, FMA} x {fast, robust}: hits and occluded byte for byte (FMA scenes prepared with ARITH_FMA)."""
    rays = tc.adversarial_rays()
    for mode, arith in tc.modes(gpu):
        hc, oc, _ = scenes.cpu(tc.DRAGON, arith).trace(rays, mode=mode, closest=True, occluded=True)
        for stats in (False, True):
            hg, og, st = scenes(tc.DRAGON, arith, stats).trace(rays, mode=mode, closest=True, occluded=True)
            assert tc.hits_equal(hg, hc), (mode, stats)
            assert np.array_equal(og, oc), (mode, stats)
            assert st["rays"] == len(rays) and st["hits"] == int((hc["prim"] >= 0).sum())


@pytest.mark.parametrize("name", tc.TINY_FIXTURES)
def test_gpu_equals_cpu_on_the_smallest_trees(gpu, scenes, name):
    """tri1 (the root is a leaf: the walks' root-is-leaf loop, which the dragon never enters) and quad
    (a root with two leaf children) under the adversarial windows (tmin <= -1 on rays that fail a
    u / v / w stage included), unnormalised and reversed directions, a tail of 37 rays; {exact, FMA}
    x {fast, robust}, hits and occluded byte for byte."""
    rays = tc.tiny_tree_rays(name)
    assert len(rays) % 64 != 0
    open_rays = np.array(rays)
    open_rays[:, 6:8] = (0, tc.FLT_MAX)
    for mode, arith in tc.modes(gpu):
        cpu = scenes.cpu(name, arith)
        hc, oc, _ = cpu.trace(rays, mode=mode, closest=True, occluded=True)
        tc.check_tiny_tree_input(name, rays, hc, cpu.trace(open_rays, mode=mode, closest=True)[0])
        for stats in (False, True):
            hg, og, st = scenes(name, arith, stats).trace(rays, mode=mode, closest=True, occluded=True)
            assert tc.hits_equal(hg, hc), (mode, stats)
            assert np.array_equal(og, oc), (mode, stats)
            assert st["rays"] == len(rays) and st["hits"] == int((hc["prim"] >= 0).sum())


def test_gpu_equals_cpu_on_reversed_camera_rays_of_proc_101(gpu, scenes):
    """proc_101: other stack widths / bounds than the dragon; its camera rays in reverse order."""
    name = "proc_101"
    for mode, arith in tc.modes(gpu):
        cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(name, arith)
        rays = np.ascontiguousarray(gpu.camera_rays(basis, cfg["W"], cfg["H"])[::-1])
        hc, oc, sc = scenes.cpu(name, arith).trace(rays, mode=mode, closest=True, occluded=True)
        hg, og, sg = scenes(name, arith).trace(rays, mode=mode, closest=True, occluded=True)
        assert tc.hits_equal(hg, hc) and np.array_equal(og, oc), mode
        assert sg["hits"] == sc["hits"] > 0


def test_gpu_equals_cpu_with_24_bit_stack_entries(gpu):
    """A 300 x 300 heightfield (about 94,000 sibling pairs: node indices past 16 bits, so the LDS stacks
    are the 24-bit planes) under proc_101's camera: reversed camera rays with windows from the
    adversarial set's values, a tail of 51 rays; fast exact and robust FMA."""
    cfg = dict(gpu.configs.CONFIGS["proc_101"])
    cfg["proc"] = 300
    for mode, arith in ((0, gpu.ARITH_EXACT), (gpu.MODE_FMA | gpu.MODE_ROBUST, gpu.ARITH_FMA)):
        mesh, bvh, cam = gpu.prepare(cfg, arith=arith)
        rays = np.ascontiguousarray(gpu.camera_rays(cam.basis(cfg["W"], cfg["H"]), cfg["W"], cfg["H"])[::-1][:-13])
        k = np.arange(len(rays))
        rays[:, 6] = np.asarray([0, -2, -np.inf, 1e-3], np.float32)[k % 4]
        rays[:, 7] = np.asarray([tc.FLT_MAX, np.inf, 1, 0], np.float32)[(k // 4) % 4]
        sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
        try:
            assert (1 << 16) <= sc.info()["n_pairs"] < (1 << 24)
            hc, oc, _ = cpu.trace(rays, mode=mode, closest=True, occluded=True)
            hg, og, st = sc.trace(rays, mode=mode, closest=True, occluded=True)
            assert tc.hits_equal(hg, hc) and np.array_equal(og, oc), mode
            assert st["hits"] == int(oc.sum()) > 10000
        finally:
            sc.close()
            cpu.close()


@pytest.fixture(scope="module")
def ray_scenes(gpu):
    """get(set, arith, stats) -> the Scene of a ray set's scene (tests/golden/rays/<set>.npz), created once."""
    cache = {}

    def get(name, arith=0, stats=False):
        key = ("proc300" if name == "proc300_window" else tc.ray_set_config(name)["obj"], arith, stats)
        if key not in cache:
            cache[key] = gpu.Scene(*tc.ray_set_scene(name, arith), stats=stats)
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_caller_rays_equal_the_reference_traverser(gpu, ray_scenes, name, variant):
    """Every stored ray, the non-finite ones included, against the reference's own
    traverse(ray, intersector): the production kernel in stored order (dragon_octants: the eight
    octant loops, the group with one odd lane, the uniform tail), with both queries, closest only
    and occluded only (three instantiations); the stats kernel in stored order, and split into the
    rays without and with a NaN for the Statistics."""
    arith = tc.variant_mode(gpu, variant)[1]
    prod, st = tracer(ray_scenes(name, arith)), tracer(ray_scenes(name, arith, stats=True))
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False)
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False, occluded=False)
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False, closest=False)
    tc.check_against_ray_fixture(gpu, st, name, variant, stats=False)
    tc.check_against_ray_fixture(gpu, st, name, variant, stats=True)


OCTANTS = "dragon_octants"


@pytest.mark.parametrize("variant", ["exact_fast", "ref_fast"])
def test_octant_loops_equal_the_generic_loop_under_a_permutation(gpu, ray_scenes, variant):
    """dragon_octants in stored order (uniform wavefronts: the kOct 0..7 loops) and under a
    permutation that leaves no wavefront uniform (the generic loop): the same bytes ray by ray, and
    both the reference's."""
    rays = tc.load_ray_fixture(OCTANTS)["rays"]
    mode, arith = tc.variant_mode(gpu, variant)
    sc = ray_scenes(OCTANTS, arith)
    perm = np.random.default_rng(20261022).permutation(len(rays))
    octant = tc.ray_octant(rays)[perm]
    for k in range(0, len(rays), 64):
        assert len(set(octant[k:k + 64].tolist())) > 1, k             # every wavefront of the permuted run is mixed
    h0, o0, _ = sc.trace(rays, mode=mode, closest=True, occluded=True)
    h1, o1, _ = sc.trace(np.ascontiguousarray(rays[perm]), mode=mode, closest=True, occluded=True)
    back_h, back_o = np.empty_like(h1), np.empty_like(o1)
    back_h[perm], back_o[perm] = h1, o1
    assert tc.hits_equal(back_h, h0) and np.array_equal(back_o, o0)
    tc.check_against_ray_fixture(gpu, tracer(sc), OCTANTS, variant, stats=False)
    tc.check_against_ray_fixture(gpu, tracer(sc), OCTANTS, variant, stats=False, select=perm)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
def test_lattice_ties_in_octant_order(gpu, ray_scenes, variant):
    """lattice_ties a second time, stably sorted by octant: at least four whole wavefronts of every
    octant are uniform and take the kOct 0..7 loops of the fast walks (the robust walks have one
    loop; they see the same rays in other wavefronts), where the stored order -- no uniform
    wavefront, asserted -- takes the generic loop.  Exact ties in u, v, w, t = tmin, t = tmax and
    coincident triangles must come out the reference's way in each."""
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    octant = tc.ray_octant(rays)
    order = tc.lattice_octant_order(rays)
    assert not tc.uniform_wavefronts(octant).any()
    assert (tc.uniform_wavefronts(octant[order]) >= 4).all()
    assert np.array_equal(np.sort(order), np.arange(len(rays))) and (np.diff(octant[order]) >= 0).all()
    arith = tc.variant_mode(gpu, variant)[1]
    prod, st = tracer(ray_scenes(tc.LATTICE, arith)), tracer(ray_scenes(tc.LATTICE, arith, stats=True))
    tc.check_against_ray_fixture(gpu, prod, tc.LATTICE, variant, stats=False, select=order)
    tc.check_against_ray_fixture(gpu, prod, tc.LATTICE, variant, stats=False, occluded=False, select=order)
    tc.check_against_ray_fixture(gpu, prod, tc.LATTICE, variant, stats=False, closest=False, select=order)
    tc.check_against_ray_fixture(gpu, st, tc.LATTICE, variant, stats=True, select=order)


@pytest.mark.parametrize("variant", ["exact_fast", "ref_fast"])
def test_octant_loops_on_a_uniform_tail_wavefront(gpu, ray_scenes, variant):
    """trace_device on prefixes of dragon_octants whose last wavefront holds 37 rays of one octant
    (groups 3 and 20: octants 1 and 6; the whole set: octant 3): the first n results of the full
    run, which are the reference's, and the 64 entries behind each output buffer untouched."""
    import torch
    fx = tc.load_ray_fixture(OCTANTS)
    rays, ref = fx["rays"], fx[variant]
    mode, arith = tc.variant_mode(gpu, variant)
    sc = ray_scenes(OCTANTS, arith)
    full_h, full_o, _ = sc.trace(rays, mode=mode, closest=True, occluded=True)
    assert tc.hits_equal(full_h, tc.reference_hits(gpu, ref)) and np.array_equal(full_o, ref["occluded"])
    octant = tc.ray_octant(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for k in (3, 20, 25):
        n = 64 * k + 37
        assert n <= len(rays) and len(set(octant[64 * k:n].tolist())) == 1
        d_hits = torch.full((n + 64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_occ = torch.full((n + 64,), 0xa5, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        sc.trace_device(d_rays.data_ptr(), n, mode=mode, d_hits16=d_hits.data_ptr(), d_occluded=d_occ.data_ptr(),
                        d_counters=d_cnt.data_ptr(), stream=st)
        torch.cuda.synchronize()
        h, o, c = d_hits.cpu().numpy(), d_occ.cpu().numpy(), d_cnt.cpu().numpy()
        assert h[:n].tobytes() == full_h[:n].tobytes(), n
        assert np.array_equal(o[:n], full_o[:n]), n
        assert (h[n:] == 0x5a5a5a5a).all() and (o[n:] == 0xa5).all(), n
        assert c[0] == n and c[1] == int((ref["prim"][:n] >= 0).sum()) and c[6] == 0, n


def test_tails_and_guard_regions(gpu, scenes):
    """n_rays that does not fill the last wavefront: the first n results of the full run, and the 64
    entries behind each output buffer untouched."""
    import torch
    rays = tc.adversarial_rays()
    sc = scenes(tc.DRAGON)
    full_h, full_o, _ = sc.trace(rays, closest=True, occluded=True)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n in (1, 63, 64, 65, 4097):
        d_hits = torch.full((n + 64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_occ = torch.full((n + 64,), 0xa5, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        sc.trace_device(d_rays.data_ptr(), n, d_hits16=d_hits.data_ptr(), d_occluded=d_occ.data_ptr(),
                        d_counters=d_cnt.data_ptr(), stream=st)
        torch.cuda.synchronize()
        h, o, c = d_hits.cpu().numpy(), d_occ.cpu().numpy(), d_cnt.cpu().numpy()
        assert h[:n].tobytes() == full_h[:n].tobytes(), n
        assert np.array_equal(o[:n], full_o[:n]), n
        assert (h[n:] == 0x5a5a5a5a).all() and (o[n:] == 0xa5).all(), n
        assert c[0] == n and c[1] == int((full_h["prim"][:n] >= 0).sum()) and c[6] == 0, n


def test_device_call_on_two_streams(gpu, scenes):
    """Two trace_device calls of one scene on two streams (one half of the rays each), one
    synchronise: the host call's results; d_counters rays and hits of each half."""
    import torch
    rays = tc.adversarial_rays()
    sc = scenes(tc.DRAGON)
    full_h, full_o, _ = sc.trace(rays, closest=True, occluded=True)
    n = len(rays)
    cut = 2048                                                        # a multiple of 64: 32-B records stay 16-B aligned anyway
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
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


def test_direction_scale(gpu, scenes):
    tc.check_scale(gpu, tracer(scenes(tc.DRAGON)))


def test_window(gpu, scenes):
    tc.check_window(gpu, tracer(scenes(tc.DRAGON)))
    tc.check_window(gpu, tracer(scenes(tc.DRAGON, stats=True)))


def test_interface_details(gpu, scenes):
    import ctypes
    sc = scenes(tc.DRAGON)
    rays = np.array(tc.adversarial_rays()[:4])
    h0, o0, st = sc.trace(np.zeros((0, 8), np.float32), closest=True, occluded=True)
    assert len(h0) == 0 and len(o0) == 0 and st["rays"] == 0
    for bad in (gpu.MODE_PRIMARY, gpu.MODE_QBVH4, gpu.MODE_FMA | gpu.MODE_PRIMARY):
        with pytest.raises(gpu.CeresError, match="error -1"):
            sc.trace(rays, mode=bad)
    with pytest.raises(gpu.CeresError, match="error -1"):
        sc.trace(rays, closest=False, occluded=False)
    L = gpu.lib()
    h = np.zeros(4, gpu.HIT_DTYPE)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    assert L.ceres_trace_rays(sc._h, vp(rays), 1 << 31, 0, vp(h), None, None) == -6
    cfg = gpu.configs.CONFIGS["tri1"]
    mesh, bvh, _ = gpu.prepare(cfg, f64=True)
    d = gpu.Scene(mesh, bvh)
    try:
        assert L.ceres_trace_rays(d._h, vp(rays), 4, 0, vp(h), None, None) == -6
    finally:
        d.close()


def test_render_is_undisturbed_by_trace_calls(gpu):
    """After trace calls on a scene, Scene.render of dragon_333x217 still gives the fixture's PPM, in
    both arithmetics: the ray queries share the scene's buffers, not its cached launch state."""
    rays = tc.adversarial_rays()
    for build, arith in (("exact", gpu.ARITH_EXACT), ("ref", gpu.ARITH_FMA)):
        cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(tc.DRAGON, arith)
        sc = gpu.Scene(mesh, bvh)
        try:
            W, H = cfg["W"], cfg["H"]
            mode = gpu.cfg_mode(cfg, arith)
            sc.trace(rays, mode=mode & gpu.MODE_FMA, closest=True, occluded=True)
            _, rgb, st = sc.render(basis, sun, W, H, mode=mode)
            assert hashlib.sha256(gpu.ppm(W, H, rgb)).hexdigest() == meta["ppm_sha256"][build], build
            assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"])
            sc.trace(rays, mode=mode & gpu.MODE_FMA, closest=True, occluded=True)
            _, rgb2, _ = sc.render(basis, sun, W, H, mode=mode)
            assert np.array_equal(rgb, rgb2)
        finally:
            sc.close()
