"""All-hits ray queries on the GPU (ceres_trace_all_k behind ceres_trace_rays_all / _device, Scene.trace_all,
`./render --rays --all-hits`): every hit in a ray's window, in order.  Two bars.  The reference's own answer
(tests/golden/rays_all/: its traverser run with a collecting intersector that never lowers ray.tmax), compared
directly: counts, rows of 32, 5 and 1 records and the count-only kernel bit for bit on production and stats
scenes, in the four variants, on the eight ray sets, on dupleaf_stack (rows past 32 records of one t: order and
eviction by original index; also at the three stack widths and through the device call at 63, 64 and 65 rays)
and on four non-finite soups (host- and GPU-built trees); on stats scenes node_pairs and tri_tests are the
reference's summed Statistics.  And the CPU path (ceres_trace_rays_all_cpu), which tests/test_allhits_cpu.py
pins to the same files and to a model of the walk: the same comparisons, then the three stack widths, the
deepest trees (stack plus hit list largest), tails, the device call on two streams, the CLI, and scenes
changed in place -- refit, rebuild, update either way -- or created from device arrays."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import allhits_common as ac
import refit_common as rc
import trace_common as tc

pytestmark = pytest.mark.gpu

ENV = "CERES_DEBUG_STACK_WIDTH"
KS = (1, 5, ac.MAX_HITS)


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def scenes(gpu):
    """get(set, arith, stats) -> Scene, get.cpu(set, arith) -> CpuScene, created once per module."""
    cache = {}

    def key_of(name, arith):
        return (ac.scene_key(name), arith)

    class Get:
        def __call__(self, name, arith=0, stats=False):
            key = key_of(name, arith) + (stats,)
            if key not in cache:
                cache[key] = gpu.Scene(*ac.all_set_scene(name, arith), stats=stats)
            return cache[key]

        def cpu(self, name, arith=0):
            key = key_of(name, arith) + ("cpu",)
            if key not in cache:
                cache[key] = gpu.CpuScene(*ac.all_set_scene(name, arith))
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def expected(scenes):
    """get(set, mode, arith) -> the CPU path's {K: (counts, rows)} for K in KS, stats; computed once."""
    cache = {}

    def get(name, mode, arith):
        key = (name, mode, arith)
        if key not in cache:
            rays = tc.load_ray_fixture(name)["rays"]
            out = {}
            for K in KS:
                c, r, st = scenes.cpu(name, arith).trace_all(rays, max_hits=K, mode=mode)
                out[K] = (c, r)
            out["stats"] = st
            cache[key] = out
        return cache[key]

    return get


def assert_same(got, exp, where):
    (c, r), (ec, er) = got, exp
    assert np.array_equal(c, ec), (where, "counts", np.flatnonzero(c != ec)[:8])
    if er is not None:
        bad = np.flatnonzero((r.view(np.uint32) != er.view(np.uint32)).reshape(len(er), -1).any(axis=1))
        assert ac.rows_equal(r, er), (where, "first differing rays", bad[:8])


def check_scene_against_cpu(sc, exp, rays, mode, where, stats):
    for K in KS:
        c, r, st = sc.trace_all(rays, max_hits=K, mode=mode)
        assert_same((c, r), exp[K], where + (K,))
        assert st["rays"] == len(rays) and st["hits"] == exp["stats"]["hits"], where
        if stats:
            assert (st["node_pairs"], st["tri_tests"]) == (exp["stats"]["node_pairs"], exp["stats"]["tri_tests"]), where + (K,)
    c, r, st = sc.trace_all(rays, max_hits=0, mode=mode, hits=False)
    assert r is None and np.array_equal(c, exp[1][0]), where + ("count-only",)
    assert st["hits"] == exp["stats"]["hits"]
    if stats:
        assert (st["node_pairs"], st["tri_tests"]) == (exp["stats"]["node_pairs"], exp["stats"]["tri_tests"]), where


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_gpu_equals_cpu_path(gpu, scenes, expected, name, variant):
    """Counts and rows bit for bit at max_hits 1, 5, 32 and count-only, production and stats scenes; stats
    scenes: node_pairs and tri_tests equal the CPU path's."""
    mode, arith = tc.variant_mode(gpu, variant)
    rays = tc.load_ray_fixture(name)["rays"]
    exp = expected(name, mode, arith)
    for stats in (False, True):
        check_scene_against_cpu(scenes(name, arith, stats), exp, rays, mode, (name, variant, "stats" if stats else "production"), stats)


def gpu_tracer(scene):
    return lambda rays, max_hits, mode, hits: scene.trace_all(rays, max_hits=max_hits, mode=mode, hits=hits)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", ac.ALL_SETS)
def test_gpu_equals_the_reference_traversers_all_hits(gpu, scenes, name, variant):
    """Against tests/golden/rays_all/ directly: counts and rows at max_hits 32, the rows of 1 and 5 as prefixes
    and the count-only kernel, bit for bit, on a production and a stats scene; on the stats scene node_pairs
    and tri_tests are the reference's summed traversal_steps and intersections."""
    _, arith = tc.variant_mode(gpu, variant)
    for stats in (False, True):
        ac.check_against_all_fixture(gpu, gpu_tracer(scenes(name, arith, stats)), name, variant, stats=stats)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", list(ac.SOUP_SETS))
def test_soups_over_gpu_built_trees(gpu, name, variant):
    """The soup sets again on scenes whose BVH build_bvh_gpu made (test_gpu_soups.py pins the trees equal)."""
    _, arith = tc.variant_mode(gpu, variant)
    mesh, _ = ac.all_set_scene(name, arith)
    bvh = gpu.build_bvh_gpu(mesh, arith=arith)
    for stats in (False, True):
        sc = gpu.Scene(mesh, bvh, stats=stats)
        try:
            ac.check_against_all_fixture(gpu, gpu_tracer(sc), name, variant, stats=stats, prefixes=(5,))
        finally:
            sc.close()


@contextlib.contextmanager
def forced(width):
    """CERES_DEBUG_STACK_WIDTH while a scene is created; the environment is restored."""
    old = os.environ.pop(ENV, None)
    os.environ[ENV] = str(width)
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("name", [tc.LATTICE, "quad_tiny"])
def test_widened_stack_entries_change_nothing(gpu, scenes, expected, name, width):
    """The 24- and 32-bit-stack instantiations on small scenes (the hook, set while the scene is made)."""
    rays = tc.load_ray_fixture(name)["rays"]
    for mode, arith in ((0, gpu.ARITH_EXACT), (gpu.MODE_FMA | gpu.MODE_ROBUST, gpu.ARITH_FMA)):
        exp = expected(name, mode, arith)
        for stats in (False, True):
            with forced(width):
                sc = gpu.Scene(*tc.ray_set_scene(name, arith), stats=stats)
            try:
                assert sc.stack_width() == width
                check_scene_against_cpu(sc, exp, rays, mode, (name, width, mode, stats), stats)
            finally:
                sc.close()


@pytest.mark.parametrize("width", [2, 3, 4])
def test_dupleaf_stack_at_the_three_stack_widths(gpu, scenes, width):
    """Rows past 32 records of one t against the stored reference answers in the 16-, 24- and 32-bit-stack
    instantiations (2 is the scene's own width; 3 and 4 by the hook, set while the scene is made)."""
    for variant in ("exact_fast", "ref_robust"):
        _, arith = tc.variant_mode(gpu, variant)
        for stats in (False, True):
            if width == 2:
                sc = scenes(ac.DUPLEAF, arith, stats)
            else:
                with forced(width):
                    sc = gpu.Scene(*ac.all_set_scene(ac.DUPLEAF, arith), stats=stats)
            try:
                assert sc.stack_width() == width
                ac.check_against_all_fixture(gpu, gpu_tracer(sc), ac.DUPLEAF, variant, stats=stats, prefixes=(5,))
            finally:
                if width != 2:
                    sc.close()


def test_dupleaf_stack_tails_through_the_device_call(gpu, scenes):
    """The first 63, 64 and 65 rays of dupleaf_stack through trace_all_device at max_hits = 32: the stored
    reference rows and counts, and the sentinel-filled memory behind each output untouched."""
    import torch
    fx = ac.load_all_fixture(ac.DUPLEAF)
    ref = fx["exact_fast"]
    sc = scenes(ac.DUPLEAF)
    K = ac.MAX_HITS
    assert (ref["count"][:63] > K).any() and (ref["count"][:63] == 0).any()
    d_rays = torch.from_numpy(np.array(fx["rays"])).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n in (63, 64, 65):
        d_rows = torch.full(((n + 64) * K, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((n + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
        sc.trace_all_device(d_rays.data_ptr(), n, max_hits=K, d_counts=d_cnt.data_ptr(), d_hits16=d_rows.data_ptr(),
                            d_counters=d_ctr.data_ptr(), stream=st)
        torch.cuda.synchronize()
        rows, cnt, ctr = d_rows.cpu().numpy(), d_cnt.cpu().numpy(), d_ctr.cpu().numpy()
        assert rows[:n * K].tobytes() == np.ascontiguousarray(ref["rows"][:n]).tobytes(), n
        assert np.array_equal(cnt[:n].view(np.uint32), ref["count"][:n]), n
        assert (rows[n * K:] == 0x5a5a5a5a).all() and (cnt[n:] == 0x5a5a5a5a).all(), n
        assert ctr[0] == n and ctr[1] == int((ref["count"][:n] >= 1).sum()) and ctr[2] == n and ctr[6] == 0, n


def test_native_24_bit_stack(gpu, scenes):
    """proc300_window (test_gpu_equals_cpu_path runs it) takes the 24-bit planes by itself."""
    assert scenes("proc300_window").stack_width() == 3 and scenes(tc.LATTICE).stack_width() == 2


@pytest.mark.parametrize("name", list(tc.DEEP_SETS))
def test_deep_trees_with_the_longest_list(gpu, scenes, expected, name):
    """BVHs of 52 and 53 levels at max_hits = 32: the largest stack-plus-list LDS block; the rows hold real
    work (rays with more than one hit) and no call reports a stack overflow (it would raise)."""
    rays = tc.load_ray_fixture(name)["rays"]
    sc = scenes(name)
    assert sc.info()["depth"] >= 52
    exp = expected(name, 0, 0)
    c, r, _ = sc.trace_all(rays, max_hits=ac.MAX_HITS)
    assert_same((c, r), exp[ac.MAX_HITS], (name,))
    assert (c > 1).any() and (c == 0).any()
    ac.check_rows(rays, c, r, ac.MAX_HITS)


def test_tails_and_tiny_launches(gpu, scenes, expected):
    """The first 1, 63, 64 and 65 rays of lattice_ties through the device call: the full run's first n
    answers, the memory behind each output untouched, d_counters rays and rays-with-a-hit."""
    import torch
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    sc = scenes(tc.LATTICE)
    K = 5
    full_c, full_r = expected(tc.LATTICE, 0, 0)[K]
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n in (1, 63, 64, 65):
        d_rows = torch.full(((n + 64) * K, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((n + 64,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
        sc.trace_all_device(d_rays.data_ptr(), n, max_hits=K, d_counts=d_cnt.data_ptr(), d_hits16=d_rows.data_ptr(),
                            d_counters=d_ctr.data_ptr(), stream=st)
        torch.cuda.synchronize()
        rows, cnt, ctr = d_rows.cpu().numpy(), d_cnt.cpu().numpy(), d_ctr.cpu().numpy()
        assert rows[:n * K].tobytes() == full_r[:n].tobytes(), n
        assert np.array_equal(cnt[:n].view(np.uint32), full_c[:n]), n
        assert (rows[n * K:] == 0x5a5a5a5a).all() and (cnt[n:] == 0x5a5a5a5a).all(), n
        assert ctr[0] == n and ctr[1] == int((full_c[:n] >= 1).sum()) and ctr[2] == n and ctr[6] == 0, n


def test_device_call_on_two_streams(gpu, scenes, expected):
    """Two trace_all_device calls of one scene in flight on two non-default streams, each with its own
    counters (one with rows, one count-only); then the refusals of the device call."""
    import torch
    name = "dragon_octants"
    rays = tc.load_ray_fixture(name)["rays"]
    sc = scenes(name)
    K = 5
    full_c, full_r = expected(name, 0, 0)[K]
    n, cut = len(rays), 1024
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_rows = torch.zeros((n * K, 4), dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_cnt2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ctr = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    sc.trace_all_device(d_rays.data_ptr(), cut, max_hits=K, d_counts=d_cnt.data_ptr(), d_hits16=d_rows.data_ptr(),
                        d_counters=d_ctr[0].data_ptr(), stream=s0.cuda_stream)
    sc.trace_all_device(d_rays[cut:].data_ptr(), n - cut, max_hits=K, d_counts=d_cnt[cut:].data_ptr(),
                        d_hits16=d_rows[cut * K:].data_ptr(), d_counters=d_ctr[1].data_ptr(), stream=s1.cuda_stream)
    torch.cuda.synchronize()
    sc.trace_all_device(d_rays.data_ptr(), n, d_counts=d_cnt2.data_ptr(), stream=s1.cuda_stream)      # count-only, no counters
    torch.cuda.synchronize()
    assert d_rows.cpu().numpy().tobytes() == full_r.tobytes()
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), full_c)
    assert np.array_equal(d_cnt2.cpu().numpy().view(np.uint32), full_c)
    c = d_ctr.cpu().numpy()
    assert (c[0, 0], c[0, 1]) == (cut, int((full_c[:cut] >= 1).sum())) and (c[1, 0], c[1, 1]) == (n - cut, int((full_c[cut:] >= 1).sum()))
    assert c[0, 6] == 0 and c[1, 6] == 0
    # refusals: misaligned rays, hits, counts; a hit buffer with max_hits 0 or 33; neither output
    EINVAL = "error -1"
    for kw in (dict(d_rays32=d_rays.data_ptr() + 4, d_hits16=d_rows.data_ptr()), dict(d_rays32=d_rays.data_ptr(), d_hits16=d_rows.data_ptr() + 8),
               dict(d_rays32=d_rays.data_ptr(), d_hits16=d_rows.data_ptr(), d_counts=d_cnt.data_ptr() + 2)):
        with pytest.raises(gpu.CeresError, match=EINVAL):
            sc.trace_all_device(n_rays=64, max_hits=K, stream=s0.cuda_stream, **kw)
    for K_bad in (0, 33):
        with pytest.raises(gpu.CeresError, match=EINVAL):
            sc.trace_all_device(d_rays.data_ptr(), 64, max_hits=K_bad, d_hits16=d_rows.data_ptr(), stream=s0.cuda_stream)
    with pytest.raises(gpu.CeresError, match=EINVAL):
        sc.trace_all_device(d_rays.data_ptr(), 64, max_hits=K, stream=s0.cuda_stream)
    torch.cuda.synchronize()
    assert d_rows.cpu().numpy().tobytes() == full_r.tobytes()         # the refused calls wrote nothing


def test_host_call_refusals(gpu, scenes):
    """Each argument rule returns its status before any launch; a double scene: CERES_EUNSUPPORTED; n_rays = 0
    succeeds with zeroed stats; the closest query answers identically afterwards."""
    name = "dragon_adversarial"
    sc = scenes(name)
    rays = np.ascontiguousarray(tc.load_ray_fixture(name)["rays"][:64])
    before = sc.trace(rays, closest=True, occluded=True)
    L = gpu.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    cnt = np.zeros(64, np.uint32)
    rows = np.zeros((64, 33), gpu.HIT_DTYPE)
    call = lambda n, mode, K, c, h: L.ceres_trace_rays_all(sc._h, vp(rays), n, mode, K, c, h, None)   # noqa: E731
    assert call(64, 0, 0, vp(cnt), vp(rows)) == -1 and call(64, 0, 33, vp(cnt), vp(rows)) == -1
    assert call(64, 0, 8, None, None) == -1
    for bad in (gpu.MODE_PRIMARY, gpu.MODE_QBVH4, 0x80):
        assert call(64, bad, 8, vp(cnt), vp(rows)) == -1, bad
    assert call(1 << 31, 0, 8, vp(cnt), vp(rows)) == -6
    assert not cnt.any() and not rows.view(np.uint32).any()
    st = gpu._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    assert L.ceres_trace_rays_all(sc._h, None, 0, 0, 8, vp(cnt), vp(rows), ctypes.byref(st)) == 0
    assert (st.rays, st.hits, st.node_pairs, st.tri_tests) == (0, 0, 0, 0)
    mesh, bvh, _ = gpu.prepare(gpu.configs.CONFIGS["tri1"], f64=True)
    d = gpu.Scene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_all(d._h, vp(rays), 64, 0, 8, vp(cnt), vp(rows), None) == -6
        assert L.ceres_trace_rays_all_device(d._h, ctypes.c_void_p(256), 64, 0, 8, ctypes.c_void_p(256), ctypes.c_void_p(256), None, None) == -6
    finally:
        d.close()
    after = sc.trace(rays, closest=True, occluded=True)
    assert tc.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_after_a_refit(gpu):
    """Scene.refit with a moved mesh, then trace_all: equal to a CPU scene refitted the same way, and not to
    the answers before the move."""
    name = rc.SCENES[0]
    mesh, bvh, moved, _ = rc.moved_scene_inputs(gpu, name)
    basis, _, W, H, _ = rc.pose_of(gpu, name)
    rays = np.ascontiguousarray(gpu.camera_rays(basis, W, H)[::3])
    k = np.arange(len(rays))
    rays[:, 6] = tc.WINDOW_TMIN[k % 4]
    sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
    try:
        c0, r0, _ = sc.trace_all(rays, max_hits=8)
        assert_same((c0, r0), cpu.trace_all(rays, max_hits=8)[:2], (name, "before"))
        sc.refit(moved)
        cpu.refit(moved)
        c1, r1, _ = sc.trace_all(rays, max_hits=8)
        assert_same((c1, r1), cpu.trace_all(rays, max_hits=8)[:2], (name, "after"))
        assert (c1 > 1).any() and not ac.rows_equal(r0, r1)
    finally:
        sc.close()
        cpu.close()


def device_scene(pkg, mesh):
    """A Scene.from_device scene over a GPU-built BVH of `mesh` (tensors returned to keep them alive)."""
    import torch
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
    scene = pkg.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stream=stream)
    return scene, (d_tri, d_norm, d_nodes, d_prim)


# tri1: refit_common's smallest scene (a root leaf).  dupleaf, beside it: after the move its copies are still
# coincident, so the rebuilt tree has the oversized leaves and the rows are full of records equal in t.
@pytest.mark.parametrize("how", ["rebuild", "update_rebuilds", "update_refits", "from_device"])
@pytest.mark.parametrize("name", ["tri1", "dupleaf"])
def test_scenes_changed_in_place(gpu, name, how):
    """trace_all at max_hits 8 and 32 after Scene.rebuild(moved), after Scene.update(moved, max_ratio) with a
    ratio that rebuilds and one that does not, and on Scene.from_device over a GPU-built tree of the moved
    mesh: equal to a CpuScene taken through the same call and to a fresh Scene of the moved mesh (over the
    host-built tree, or the numpy-refitted one where the update only refits)."""
    mesh, bvh, moved, refitted = rc.moved_scene_inputs(gpu, name)
    basis, _, W, H, _ = rc.pose_of(gpu, name)
    rays = np.ascontiguousarray(gpu.camera_rays(basis, W, H))
    k = np.arange(len(rays))
    rays[:, 6] = tc.WINDOW_TMIN[k % 4]
    built = refitted if how == "update_refits" else gpu.build_bvh(moved)
    keep = None
    if how == "from_device":
        sc, keep = device_scene(gpu, moved)
        cpu = gpu.CpuScene(moved, built)
    else:
        sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
    fresh = gpu.Scene(moved, built)
    try:
        before = gpu.CpuScene(mesh, bvh)
        old = before.trace_all(rays, max_hits=8)[1]
        before.close()
        if how == "rebuild":
            sc.rebuild(moved)
            cpu.rebuild(moved)
        elif how != "from_device":
            ratio = 1e-9 if how == "update_rebuilds" else np.inf
            u, cu = sc.update(moved, ratio), cpu.update(moved, ratio)
            assert u["rebuilt"] == cu["rebuilt"] == (how == "update_rebuilds"), (u, cu)
        for K in (8, ac.MAX_HITS):
            c, r, _ = sc.trace_all(rays, max_hits=K)
            assert_same((c, r), cpu.trace_all(rays, max_hits=K)[:2], (name, how, K, "cpu"))
            assert_same((c, r), fresh.trace_all(rays, max_hits=K)[:2], (name, how, K, "fresh"))
            ac.check_rows(rays, c, r, K)
            assert (c >= 1).any() and (c == 0).any(), (name, how)
            if name == "dupleaf":
                assert (c > ac.MAX_HITS).any(), (name, how)
            if K == 8:
                assert not ac.rows_equal(r, old), (name, how)           # the move shows
    finally:
        sc.close()
        cpu.close()
        fresh.close()
        del keep


def test_cli_on_the_gpu(gpu, tmp_path):
    """./render --rays --all-hits K: the --cpu run's files, byte for byte."""
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    rf = tmp_path / "rays.bin"
    rf.write_bytes(rays.tobytes())
    out = {}
    for where in ("gpu", "cpu"):
        hf, cf = tmp_path / (where + "_hits.bin"), tmp_path / (where + "_counts.bin")
        args = [gpu.CLI_PATH, tc.LATTICE_OBJ, "--exact", "--rays", str(rf), "--all-hits", "8", "--hits-out", str(hf), "--counts-out", str(cf)]
        r = subprocess.run(args + (["--cpu"] if where == "cpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[where] = (hf.read_bytes(), cf.read_bytes())
    assert out["gpu"] == out["cpu"] and len(out["gpu"][0]) == len(rays) * 8 * 16 and len(out["gpu"][1]) == len(rays) * 4
    r = subprocess.run([gpu.CLI_PATH, tc.LATTICE_OBJ, "--double", "--rays", str(rf), "--all-hits", "8", "--hits-out", str(tmp_path / "x.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "float scenes" in r.stderr
