"""Closest-point queries on double scenes on the GPU (ceres_closest_points_f64, _f64_device, _f64_indexed_device;
Scene.closest_points_f64, Scene.closest_points_f64_device) against the float64 brute force of closest64_common.py,
byte for byte: the contract makes the answer the minimum over all triangles of one float64 formula, whatever the
tree and the visiting order.  Pinned here: every scene and point set (cap26: the deepest legal stack, 64
entries); tail lanes and untouched slots; the indexed call; refit; device-built double scenes; counters and statistics;
two streams; soups with non-finite triangles (status and index range only); the refusals, bracketed by renders;
equality with the CPU path."""
import ctypes

import numpy as np
import pytest

import closest64_common as c64
import closest_common as cc
import soup_common as soup

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6
FILL = 0x5a
COUNTS = (1, 63, 64, 65, 130)                                         # tail lanes; a second and a third wavefront
CAP26_DEPTH = 64                                                      # Scene.info()["depth"] of the double cap26 tree


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("closest64_gpu")


@pytest.fixture(scope="module")
def scenes(gpu, tmp):
    cache = {}

    def get(name, stats=False):
        if (name, stats) not in cache:
            cache[(name, stats)] = gpu.Scene(*c64.scene(name, tmp), stats=stats)
        return cache[(name, stats)]

    yield get
    for s in cache.values():
        s.close()


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes):
    import torch
    return torch.full((int(nbytes),), FILL, dtype=torch.uint8, device="cuda")


def device_call(sc, pts, n=None, slots=None, index=None, counters=True, stream=0):
    """One device call into a sentinel-filled buffer of `slots` records -> (records [slots] as NEAR64_DTYPE,
    counters [8] u64 | None)."""
    import torch
    n = len(pts) if n is None else n
    slots = n if slots is None else slots
    d_pts = to_device(pts)
    d_out = filled(32 * slots)
    d_cnt = torch.full((8,), 0x5a5a5a5a, dtype=torch.int64, device="cuda") if counters else None
    kw = {}
    if index is not None:
        d_idx = to_device(np.asarray(index, np.uint32)) if len(index) else torch.zeros(4, dtype=torch.uint8, device="cuda")
        kw = dict(d_index=d_idx.data_ptr(), n_index=len(index))
    sc.closest_points_f64_device(d_pts.data_ptr(), n, d_out.data_ptr(), d_counters=d_cnt.data_ptr() if counters else 0, stream=stream, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(c64.NEAR64_DTYPE), (d_cnt.cpu().numpy().view(np.uint64) if counters else None)


SENTINEL = np.frombuffer(bytes([FILL]) * 32, c64.NEAR64_DTYPE)[0]


@pytest.mark.parametrize("name", c64.SCENES)
def test_gpu_equals_the_model(gpu, scenes, tmp, name):
    """Host-array and device calls on every scene and set, and the CPU path's bytes.  cap26 is 64 levels deep:
    64 entries x 64 lanes of LDS stack -- 16 KiB of pair indices, 48 KiB if the library was built with the bound
    plane -- inside a workgroup's 64 KiB either way."""
    import torch
    sets, near = c64.expected(name, tmp)
    pts, want = c64.joined(sets), c64.joined(near)
    sc = scenes(name)
    if name == "cap26":
        info = sc.info()
        assert info["depth"] == CAP26_DEPTH and info["stack_entries"] == CAP26_DEPTH
        assert info["stack_entries"] * 64 * 12 == 48 << 10 <= torch.cuda.get_device_properties(0).shared_memory_per_block
    got, st = sc.closest_points_f64(pts)
    assert got.dtype == gpu.NEAR64_DTYPE
    assert c64.same(got, want), c64.first_difference(got, want, pts)
    found = int((want["prim"] >= 0).sum())
    assert st["rays"] == len(pts) and st["hits"] == found
    got, cnt = device_call(sc, pts)
    assert c64.same(got, want), c64.first_difference(got, want, pts)
    assert cnt.tolist() == [len(pts), found, len(pts), 0, 0, 0, 0, 0]
    got3, _ = sc.closest_points_f64(sets["a_uniform"][:, :3])             # [n, 3]: r2max = +inf
    assert c64.same(got3, near["a_uniform"])
    cpu = gpu.CpuScene(*c64.scene(name, tmp))
    host, _ = cpu.closest_points_f64(pts, threads=2)
    cpu.close()
    assert c64.same(got, host)


@pytest.mark.parametrize("name", ["quad", "bunny", "arms6"])
def test_tail_lanes_and_untouched_slots(gpu, scenes, name):
    sets, near = c64.expected(name)
    pts, want = c64.joined(sets), c64.joined(near)
    sc = scenes(name)
    for n in COUNTS:
        got, cnt = device_call(sc, pts, n=n, slots=n + 70)
        assert c64.same(got[:n], want[:n]), (n, c64.first_difference(got[:n], want[:n], pts))
        assert (got[n:] == SENTINEL).all(), n
        assert cnt[0] == n and cnt[2] == n and cnt[1] == int((want["prim"][:n] >= 0).sum()) and cnt[6] == 0
    got, _ = device_call(sc, pts, counters=False)                         # counters are optional
    assert c64.same(got, want)


@pytest.mark.parametrize("name", ["bunny", "bodyarms"])
def test_indexed(gpu, scenes, name):
    sets, near = c64.expected(name)
    pts, want = c64.joined(sets), c64.joined(near)
    n = len(pts)
    sc = scenes(name)
    rng = np.random.default_rng(11)
    for index in (np.arange(n), np.arange(n)[::-1]):
        got, cnt = device_call(sc, pts, index=index)
        assert c64.same(got, want), c64.first_difference(got, want, pts)
        assert cnt.tolist() == [n, int((want["prim"] >= 0).sum()), n, 0, 0, 0, 0, 0]
    sub = np.sort(rng.choice(n, 37, replace=False))
    got, cnt = device_call(sc, pts, index=sub)
    listed = np.zeros(n, bool)
    listed[sub] = True
    assert c64.same(got[listed], want[listed]) and (got[~listed] == SENTINEL).all()
    assert cnt[0] == 37 and cnt[1] == int((want["prim"][sub] >= 0).sum())
    wild = np.concatenate([sub[:20], [n, n + 1, 0x7fffffff, 0xffffffff], sub[20:]]).astype(np.uint32)
    got, cnt = device_call(sc, pts, index=wild)                           # entries >= n_points are skipped
    assert c64.same(got[listed], want[listed]) and (got[~listed] == SENTINEL).all()
    assert cnt[0] == len(wild) and cnt[1] == int((want["prim"][sub] >= 0).sum())
    got, cnt = device_call(sc, pts, index=np.zeros(0, np.uint32))         # n_index = 0: nothing touched
    assert (got == SENTINEL).all() and (cnt == 0x5a5a5a5a).all()


@pytest.mark.parametrize("name", ["quad", "bunny", "bodyarms"])
def test_after_refit(gpu, name):
    mesh, bvh = c64.scene(name)
    sets, near = c64.expected(name)
    pts = c64.joined(sets)
    moved = c64.moved_mesh(gpu, mesh, name)
    want = c64.model64_exact(moved.tri, pts)
    assert not c64.same(want, c64.joined(near))
    sc = gpu.Scene(mesh, bvh)
    sc.refit(moved)
    got, _ = sc.closest_points_f64(pts)
    sc.close()
    assert c64.same(got, want), c64.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["tri1", "bunny", "arms6"])
def test_device_built_scene(gpu, name):
    """Scene.from_device_f64 over the GPU-built double tree (another topology than the host builder's where ties differ)."""
    import torch
    mesh, _ = c64.scene(name)
    sets, near = c64.expected(name)
    pts, want = c64.joined(sets), c64.joined(near)
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.empty(max(2 * n - 1, 1) * 8, dtype=torch.int64, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = gpu.build_bvh_device_f64(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
    sc = gpu.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stream=stream)
    got, _ = sc.closest_points_f64(pts)
    sc.close()
    assert c64.same(got, want), c64.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["tri1", "bunny", "bodyarms"])
def test_counters_and_stats(gpu, scenes, name):
    sets, near = c64.expected(name)
    pts, want = c64.joined(sets), c64.joined(near)
    found = int((want["prim"] >= 0).sum())
    assert 0 < found < len(pts)                                           # points = found + misses, both present
    sc = scenes(name, stats=True)
    got, cnt = device_call(sc, pts)
    assert c64.same(got, want), c64.first_difference(got, want, pts)
    assert cnt[[0, 1, 2, 3, 6, 7]].tolist() == [len(pts), found, len(pts), 0, 0, 0]
    assert int(cnt[0]) == found + int((got["prim"] < 0).sum())
    assert cnt[5] >= found and cnt[5] > 0
    assert (cnt[4] > 0) == (name != "tri1")                               # a root leaf has no pair to visit
    got, st = sc.closest_points_f64(pts)
    assert c64.same(got, want)
    assert (st["rays"], st["hits"], st["node_pairs"], st["tri_tests"]) == (cnt[0], cnt[1], cnt[4], cnt[5])
    assert st["ms"] > 0
    _, st0 = scenes(name).closest_points_f64(pts)                         # a plain scene counts neither
    assert st0["node_pairs"] == 0 and st0["tri_tests"] == 0 and st0["hits"] == found


def test_two_streams_in_flight(gpu, scenes):
    import torch
    sets, near = c64.expected("bunny")
    pts, want = c64.joined(sets), c64.joined(near)
    sc = scenes("bunny")
    d_pts = to_device(pts)
    outs = [filled(32 * len(pts)) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    for _ in range(3):
        for o, s in zip(outs, streams):
            sc.closest_points_f64_device(d_pts.data_ptr(), len(pts), o.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        assert c64.same(o.cpu().numpy().view(c64.NEAR64_DTYPE), want)


@pytest.mark.parametrize("kind,n", [("mixed_nan", 4097), ("mixed", 4097)])
def test_soups_stay_in_range(gpu, kind, n):
    """Non-finite triangles (the float soups widened to double) are outside the contract: the call succeeds and
    every prim is in [-1, n_tri) -- nothing more is asserted."""
    m32 = soup.mesh_of(gpu, kind, n)
    with np.errstate(invalid="ignore"):                                   # (the soups' signalling NaNs)
        mesh = gpu.Mesh(m32.tri.astype(np.float64), m32.norm.astype(np.float64))
    assert not np.isfinite(mesh.tri).all()
    sets = c64.base_sets(soup.base(n).astype(np.float64))
    pts = np.concatenate([sets[k] for k in ("a_uniform", "c_jitter", "f_nonfinite")])
    sc = gpu.Scene(mesh, gpu.build_bvh(mesh))
    got, st = sc.closest_points_f64(pts)
    sc.close()
    assert st["rays"] == len(pts)
    assert ((got["prim"] >= -1) & (got["prim"] < n)).all()


def test_a_nan_d2_is_never_taken(gpu):
    mesh = c64.overflow_mesh(gpu)
    sets = c64.base_sets(mesh.tri[0::2])
    pts = np.concatenate([sets[k] for k in c64.ORDER[:4]])
    want = c64.model64_exact(mesh.tri, pts)
    sc = gpu.Scene(mesh, gpu.build_bvh(mesh))
    got, _ = sc.closest_points_f64(pts)
    sc.close()
    assert c64.same(got, want), c64.first_difference(got, want, pts)


def test_refusals_leave_everything_untouched(gpu, scenes):
    import torch
    L = gpu.lib()
    cfg = gpu.configs.CONFIGS["quad"]
    _, _, cam = gpu.prepare(cfg, f64=True)
    _, sun = gpu.pose_f64(cfg)
    sc = scenes("quad")
    before = sc.render(cam.basis(64, 48), sun, 64, 48)[0].copy()
    pts = np.ascontiguousarray(c64.expected("quad")[0]["a_uniform"])
    n = len(pts)
    d_pts, d_out = to_device(pts), filled(32 * n + 32)
    d_cnt = torch.full((8,), 0x5a5a5a5a, dtype=torch.int64, device="cuda")
    p, o, c = d_pts.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    call = L.ceres_closest_points_f64_device
    assert call(None, p, n, o, c, None) == EINVAL and b"null scene" in L.ceres_last_error()
    assert call(sc._h, None, n, o, c, None) == EINVAL
    assert call(sc._h, p, n, None, c, None) == EINVAL
    assert call(sc._h, p + 8, n - 1, o, c, None) == EINVAL and b"16-byte aligned" in L.ceres_last_error()
    assert call(sc._h, p, n - 1, o + 8, c, None) == EINVAL
    assert call(sc._h, p, 1 << 31, o, c, None) == EUNSUPPORTED
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    icall = L.ceres_closest_points_f64_indexed_device
    assert icall(sc._h, p, n, None, n, o, c, None) == EINVAL
    assert icall(sc._h, p, n, idx.data_ptr() + 2, n - 1, o, c, None) == EINVAL
    assert icall(sc._h, p, n, idx.data_ptr(), 1 << 31, o, c, None) == EUNSUPPORTED
    st = scenes("quad", stats=True)
    assert icall(st._h, p, n, idx.data_ptr(), n, o, c, None) == EUNSUPPORTED and b"CERES_SCENE_STATS" in L.ceres_last_error()
    out = np.full(n, SENTINEL)
    sc32 = gpu.Scene(*cc.scene("quad"))                                   # a float scene handed to the _f64 calls
    assert call(sc32._h, p, n, o, c, None) == EUNSUPPORTED and b"_f64 closest-point calls take double scenes" in L.ceres_last_error()
    assert icall(sc32._h, p, n, idx.data_ptr(), n, o, c, None) == EUNSUPPORTED
    assert L.ceres_closest_points_f64(sc32._h, vp(pts), n, vp(out), None) == EUNSUPPORTED
    with pytest.raises(gpu.CeresError, match="double scenes"):
        sc32.closest_points_f64(pts)
    sc32.close()
    assert L.ceres_closest_points_f64(None, vp(pts), n, vp(out), None) == EINVAL
    assert L.ceres_closest_points_f64(sc._h, None, n, vp(out), None) == EINVAL
    assert L.ceres_closest_points_f64(sc._h, vp(pts), n, None, None) == EINVAL
    assert L.ceres_closest_points_f64(sc._h, vp(pts), 1 << 31, vp(out), None) == EUNSUPPORTED
    assert call(sc._h, p, 0, o, c, None) == 0                             # n_points = 0 touches nothing
    assert L.ceres_closest_points_f64(sc._h, None, 0, vp(out), None) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert (d_out.cpu().numpy() == FILL).all() and (d_cnt.cpu().numpy() == 0x5a5a5a5a).all()
    after = sc.render(cam.basis(64, 48), sun, 64, 48)[0]
    assert before.tobytes() == after.tobytes()
    got, _ = sc.closest_points_f64(pts)
    assert c64.same(got, c64.expected("quad")[1]["a_uniform"])


def test_kernel_names(gpu):
    names = gpu.lib().ceres_kernel_names().decode().split(",")
    assert "ceres_closest_points64_k" in names and "ceres_closest_points64_idx_k" in names
