"""Closest-point queries on the GPU (ceres_closest_points, _device, _indexed_device; Scene.closest_points,
Scene.closest_points_device; `./render --points --nearest-out`) against the numpy brute force of
closest_common.py, byte for byte: the contract makes the answer the minimum over all triangles of one float32
formula, whatever the tree and the visiting order.  Pinned here: every scene and point set; tail lanes and
untouched slots; the indexed call; the stack-width hook (which must not matter); refit, rebuild, update and
device-built scenes; counters and statistics; the LDS arithmetic on the deepest tree; two streams; soups
with non-finite triangles (status and index range only); the refusals; the kernel names; the CLI."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import closest_common as cc
import soup_common as soup

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -6
FILL = 0x5a
COUNTS = (1, 63, 64, 65, 130)                                         # tail lanes; a second and a third wavefront


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("closest_gpu")


@pytest.fixture(scope="module")
def scenes(gpu, tmp):
    cache = {}

    def get(name, stats=False):
        if (name, stats) not in cache:
            cache[(name, stats)] = gpu.Scene(*cc.scene(name, tmp), stats=stats)
        return cache[(name, stats)]

    yield get
    for s in cache.values():
        s.close()


@contextlib.contextmanager
def env(**kv):
    """Environment variables while a scene is created (the hooks are read then and only then)."""
    old = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(nbytes):
    import torch
    return torch.full((int(nbytes),), FILL, dtype=torch.uint8, device="cuda")


def device_call(sc, pts, n=None, slots=None, index=None, counters=True, stream=0):
    """One device call into a sentinel-filled buffer of `slots` records -> (records [slots] as NEAR_DTYPE,
    counters [8] u64 | None)."""
    import torch
    n = len(pts) if n is None else n
    slots = n if slots is None else slots
    d_pts = to_device(pts)
    d_out = filled(16 * slots)
    d_cnt = torch.full((8,), 0x5a5a5a5a, dtype=torch.int64, device="cuda") if counters else None
    kw = {}
    if index is not None:
        d_idx = to_device(np.asarray(index, np.uint32)) if len(index) else torch.zeros(4, dtype=torch.uint8, device="cuda")
        kw = dict(d_index=d_idx.data_ptr(), n_index=len(index))
    sc.closest_points_device(d_pts.data_ptr(), n, d_out.data_ptr(), d_counters=d_cnt.data_ptr() if counters else 0, stream=stream, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(cc.NEAR_DTYPE), (d_cnt.cpu().numpy().view(np.uint64) if counters else None)


SENTINEL = np.frombuffer(bytes([FILL]) * 16, cc.NEAR_DTYPE)[0]


def lds_fits(gpu, sc):
    """Whether the scene's closest-point stack -- two [entry][lane] planes of 4-byte words, stack_entries
    entries, 64 lanes -- fits a workgroup's LDS."""
    import torch
    need = max(1, sc.info()["stack_entries"]) * 64 * 8
    have = torch.cuda.get_device_properties(0).shared_memory_per_block
    return need <= have, need, have


@pytest.mark.parametrize("name", cc.SCENES)
def test_gpu_equals_the_model(gpu, scenes, tmp, name):
    """Host-array and device calls on every scene and set; cap26 (64 levels): the answers, or the documented
    refusal before any launch, whichever the LDS arithmetic gives."""
    sets, near = cc.expected(name, tmp)
    pts, want = cc.joined(sets), cc.joined(near)
    sc = scenes(name)
    fits, need, have = lds_fits(gpu, sc)
    if not fits:
        with pytest.raises(gpu.CeresError, match="%d B of LDS per workgroup \\(%d available\\)" % (need, have)):
            sc.closest_points(pts)
        return
    got, st = sc.closest_points(pts)
    assert cc.same(got, want), cc.first_difference(got, want, pts)
    assert st["rays"] == len(pts) and st["hits"] == int((want["prim"] >= 0).sum())
    got, cnt = device_call(sc, pts)
    assert cc.same(got, want), cc.first_difference(got, want, pts)
    found = int((want["prim"] >= 0).sum())
    assert cnt.tolist() == [len(pts), found, len(pts), 0, 0, 0, 0, 0]
    got3, _ = sc.closest_points(sets["a_uniform"][:, :3])                 # [n, 3]: r2max = +inf
    assert cc.same(got3, near["a_uniform"])


@pytest.mark.parametrize("name", ["quad", "bunny", "arms6"])
def test_tail_lanes_and_untouched_slots(gpu, scenes, name):
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    sc = scenes(name)
    for n in COUNTS:
        got, cnt = device_call(sc, pts, n=n, slots=n + 70)
        assert cc.same(got[:n], want[:n]), (n, cc.first_difference(got[:n], want[:n], pts))
        assert (got[n:] == SENTINEL).all(), n
        assert cnt[0] == n and cnt[2] == n and cnt[1] == int((want["prim"][:n] >= 0).sum()) and cnt[6] == 0
    got, _ = device_call(sc, pts, counters=False)                         # counters are optional
    assert cc.same(got, want)


@pytest.mark.parametrize("name", ["bunny", "bodyarms"])
def test_indexed(gpu, scenes, name):
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    n = len(pts)
    sc = scenes(name)
    rng = np.random.default_rng(11)
    for index in (np.arange(n), np.arange(n)[::-1]):
        got, cnt = device_call(sc, pts, index=index)
        assert cc.same(got, want), cc.first_difference(got, want, pts)
        assert cnt.tolist() == [n, int((want["prim"] >= 0).sum()), n, 0, 0, 0, 0, 0]
    sub = np.sort(rng.choice(n, 37, replace=False))
    got, cnt = device_call(sc, pts, index=sub)
    listed = np.zeros(n, bool)
    listed[sub] = True
    assert cc.same(got[listed], want[listed]) and (got[~listed] == SENTINEL).all()
    assert cnt[0] == 37 and cnt[1] == int((want["prim"][sub] >= 0).sum())
    wild = np.concatenate([sub[:20], [n, n + 1, 0x7fffffff, 0xffffffff], sub[20:]]).astype(np.uint32)
    got, cnt = device_call(sc, pts, index=wild)                           # entries >= n_points are skipped
    assert cc.same(got[listed], want[listed]) and (got[~listed] == SENTINEL).all()
    assert cnt[0] == len(wild) and cnt[1] == int((want["prim"][sub] >= 0).sum())
    got, cnt = device_call(sc, pts, index=np.zeros(0, np.uint32))         # n_index = 0: nothing touched
    assert (got == SENTINEL).all() and (cnt == 0x5a5a5a5a).all()


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("name", ["bunny", "arms6"])
def test_the_stack_width_hook_does_not_matter(gpu, name, width):
    """CERES_DEBUG_STACK_WIDTH widens the ray walks' LDS stack entries; the closest-point walk keeps its own
    4-byte planes, so a scene created under the hook answers the same bytes."""
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    with env(CERES_DEBUG_STACK_WIDTH=width):
        sc = gpu.Scene(*cc.scene(name))
    assert sc.stack_width() == width
    got, _ = sc.closest_points(pts)
    sc.close()
    assert cc.same(got, want), cc.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["quad", "bunny", "bodyarms"])
def test_after_refit_rebuild_and_update(gpu, name):
    mesh, bvh = cc.scene(name)
    sets, _ = cc.expected(name)
    pts = cc.joined(sets)
    moved = cc.moved_mesh(gpu, mesh, name)
    want = cc.model32(moved.tri, pts)
    for how in ("refit", "rebuild", "update"):
        sc = gpu.Scene(mesh, bvh)
        if how == "refit":
            sc.refit(moved)
        elif how == "rebuild":
            sc.rebuild(moved)
        else:
            assert sc.update(moved, 1e-9)["rebuilt"] == 1
        got, _ = sc.closest_points(pts)
        sc.close()
        assert cc.same(got, want), (how, cc.first_difference(got, want, pts))


@pytest.mark.parametrize("name", ["tri1", "bunny", "arms6"])
def test_device_built_scene(gpu, name):
    """Scene.from_device over a GPU-built tree (another topology than the host builder's where ties differ)."""
    import torch
    mesh, _ = cc.scene(name)
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = gpu.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
    sc = gpu.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stream=stream)
    got, _ = sc.closest_points(pts)
    sc.close()
    assert cc.same(got, want), cc.first_difference(got, want, pts)


@pytest.mark.parametrize("name", ["tri1", "bunny", "bodyarms"])
def test_counters_and_stats(gpu, scenes, name):
    sets, near = cc.expected(name)
    pts, want = cc.joined(sets), cc.joined(near)
    found = int((want["prim"] >= 0).sum())
    sc = scenes(name, stats=True)
    got, cnt = device_call(sc, pts)
    assert cc.same(got, want), cc.first_difference(got, want, pts)
    assert cnt[[0, 1, 2, 3, 6, 7]].tolist() == [len(pts), found, len(pts), 0, 0, 0]
    assert cnt[5] >= found and cnt[5] > 0
    assert (cnt[4] > 0) == (name != "tri1")                               # a root leaf has no pair to visit
    got, st = sc.closest_points(pts)
    assert cc.same(got, want)
    assert (st["rays"], st["hits"], st["node_pairs"], st["tri_tests"]) == (cnt[0], cnt[1], cnt[4], cnt[5])
    assert st["ms"] > 0
    _, st0 = scenes(name).closest_points(pts)                             # a plain scene counts neither
    assert st0["node_pairs"] == 0 and st0["tri_tests"] == 0 and st0["hits"] == found


def test_two_streams_in_flight(gpu, scenes):
    import torch
    sets, near = cc.expected("bunny")
    pts, want = cc.joined(sets), cc.joined(near)
    sc = scenes("bunny")
    d_pts = to_device(pts)
    outs = [filled(16 * len(pts)) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    for _ in range(3):
        for o, s in zip(outs, streams):
            sc.closest_points_device(d_pts.data_ptr(), len(pts), o.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        assert cc.same(o.cpu().numpy().view(cc.NEAR_DTYPE), want)


@pytest.mark.parametrize("kind,n", [("mixed_nan", 4097), ("huge", 4097)])
def test_soups_stay_in_range(gpu, kind, n):
    """Non-finite triangles are outside the contract: the call succeeds and every prim is in [-1, n_tri) --
    nothing more is asserted."""
    mesh = soup.mesh_of(gpu, kind, n)
    sets = cc.base_sets(soup.base(n))
    pts = np.concatenate([sets[k] for k in ("a_uniform", "c_jitter", "f_nonfinite")])
    sc = gpu.Scene(mesh, gpu.build_bvh(mesh))
    got, st = sc.closest_points(pts)
    sc.close()
    assert st["rays"] == len(pts)
    assert ((got["prim"] >= -1) & (got["prim"] < n)).all()


def test_a_nan_d2_is_never_taken(gpu):
    mesh = cc.overflow_mesh(gpu)
    sets = cc.base_sets(mesh.tri[0::2])
    pts = np.concatenate([sets[k] for k in cc.ORDER[:4]])
    want = cc.model32(mesh.tri, pts)
    sc = gpu.Scene(mesh, gpu.build_bvh(mesh))
    got, _ = sc.closest_points(pts)
    sc.close()
    assert cc.same(got, want), cc.first_difference(got, want, pts)


def test_refusals_leave_everything_untouched(gpu, scenes):
    import torch
    L = gpu.lib()
    cfg = gpu.configs.CONFIGS["quad"]
    mesh, bvh, cam = gpu.prepare(cfg)
    sc = scenes("quad")
    before = sc.render(cam.basis(64, 48), cfg["sun"], 64, 48)[0].copy()
    pts = np.ascontiguousarray(cc.expected("quad")[0]["a_uniform"])
    n = len(pts)
    d_pts, d_out = to_device(pts), filled(16 * n + 16)
    d_cnt = torch.full((8,), 0x5a5a5a5a, dtype=torch.int64, device="cuda")
    p, o, c = d_pts.data_ptr(), d_out.data_ptr(), d_cnt.data_ptr()
    call = L.ceres_closest_points_device
    assert call(None, p, n, o, c, None) == EINVAL and b"null scene" in L.ceres_last_error()
    assert call(sc._h, None, n, o, c, None) == EINVAL
    assert call(sc._h, p, n, None, c, None) == EINVAL
    assert call(sc._h, p + 4, n - 1, o, c, None) == EINVAL and b"16-byte aligned" in L.ceres_last_error()
    assert call(sc._h, p, n - 1, o + 8, c, None) == EINVAL
    assert call(sc._h, p, 1 << 31, o, c, None) == EUNSUPPORTED
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    icall = L.ceres_closest_points_indexed_device
    assert icall(sc._h, p, n, None, n, o, c, None) == EINVAL
    assert icall(sc._h, p, n, idx.data_ptr() + 2, n - 1, o, c, None) == EINVAL
    assert icall(sc._h, p, n, idx.data_ptr(), 1 << 31, o, c, None) == EUNSUPPORTED
    st = scenes("quad", stats=True)
    assert icall(st._h, p, n, idx.data_ptr(), n, o, c, None) == EUNSUPPORTED and b"CERES_SCENE_STATS" in L.ceres_last_error()
    mesh64, bvh64, _ = gpu.prepare(cfg, f64=True)
    sc64 = gpu.Scene(mesh64, bvh64)
    assert call(sc64._h, p, n, o, c, None) == EUNSUPPORTED and b"closest-point queries take float scenes" in L.ceres_last_error()
    out = np.full(n, SENTINEL)
    assert L.ceres_closest_points(sc64._h, pts.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p), None) == EUNSUPPORTED
    sc64.close()
    assert L.ceres_closest_points(None, pts.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p), None) == EINVAL
    assert L.ceres_closest_points(sc._h, None, n, out.ctypes.data_as(ctypes.c_void_p), None) == EINVAL
    assert L.ceres_closest_points(sc._h, pts.ctypes.data_as(ctypes.c_void_p), n, None, None) == EINVAL
    assert call(sc._h, p, 0, o, c, None) == 0                                # n_points = 0 touches nothing
    assert L.ceres_closest_points(sc._h, None, 0, out.ctypes.data_as(ctypes.c_void_p), None) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert (d_out.cpu().numpy() == FILL).all() and (d_cnt.cpu().numpy() == 0x5a5a5a5a).all()
    after = sc.render(cam.basis(64, 48), cfg["sun"], 64, 48)[0]
    assert before.tobytes() == after.tobytes()
    got, _ = sc.closest_points(pts)
    assert cc.same(got, cc.expected("quad")[1]["a_uniform"])


def test_kernel_names(gpu):
    names = gpu.lib().ceres_kernel_names().decode().split(",")
    assert "ceres_closest_points_k" in names and "ceres_closest_points_idx_k" in names


def test_cli_writes_the_library_bytes(gpu, scenes, tmp):
    sets, near = cc.expected("bunny")
    pts, want = cc.joined(sets), cc.joined(near)
    cfg = gpu.configs.CONFIGS[cc.CONFIG["bunny"]]
    pfile, ofile = cc.write_points(tmp / "p.bin", pts), str(tmp / "near.bin")
    r = subprocess.run([gpu.CLI_PATH, gpu.configs.obj_path(cfg), "--rotate", cfg["rotate"][0], repr(cfg["rotate"][1]), "--exact",
                        "--points", pfile, "--nearest-out", ofile], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, _ = scenes("bunny").closest_points(pts)
    assert open(ofile, "rb").read() == got.tobytes() == want.tobytes()
    r = subprocess.run([gpu.CLI_PATH, gpu.configs.obj_path(cfg), "--double", "--points", pfile, "--nearest-out", ofile],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "closest-point queries take float scenes" in r.stderr
