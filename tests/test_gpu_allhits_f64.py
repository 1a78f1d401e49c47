"""All-hits ray queries and complete hit lists on double scenes, GPU path (ceres_trace_all64_k,
ceres_trace_lists64_k, ceres_sort_lists64_k behind ceres_trace_rays_all_f64 / _device and
ceres_trace_rays_lists_f64 / _device, Scene.trace_all / trace_lists on a double scene).

The bars are the CPU path's (tests/test_allhits_cpu_f64.py): the float64 model of the walk, bit for bit on
production and stats scenes in both variants; the reference's stored closest answers; the brute force; the
list properties; the dupleaf scene in double with the list length and the sort cap moved by the test hooks.
Then GPU against CPU byte for byte on all of dragon_adversarial64, and what only the GPU has: device calls at
wavefront tails into guarded buffers, a capacity below the total, wrong offsets, scenes changed in place and
double scenes from device arrays, the refusals."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import allhits64_common as a64
import refit_common as rc
import trace64_common as t64

pytestmark = pytest.mark.gpu

GUARD = 0x5a5a5a5a
PAD = 64                                                              # guard elements on either side of a buffer
ADV = "dragon_adversarial64"


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@pytest.fixture(scope="module")
def scenes(gpu):
    """get(set, variant, stats) -> Scene, get.cpu(set, variant) -> CpuScene, created once per module."""
    cache = {}

    class Get:
        def __call__(self, name, variant="exact_fast", stats=False):
            key = (name, a64.build_of(variant), stats)
            if key not in cache:
                cache[key] = gpu.Scene(*a64.set_scene(name, key[1]), stats=stats)
            return cache[key]

        def cpu(self, name, variant="exact_fast"):
            key = (name, a64.build_of(variant), "cpu")
            if key not in cache:
                cache[key] = gpu.CpuScene(*a64.set_scene(name, key[1]))
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


@pytest.fixture(scope="session")
def models():
    """The model's answers (allhits64_common.model is cached for the session): built here, once, so that no
    single test pays for them."""
    for name in list(a64.MODEL_SETS) + [a64.DUPLEAF64]:
        for variant in a64.VARIANTS:
            a64.model(name, variant)
    a64.model(a64.NANBOX64)
    for name in t64.BRUTE_SCENES:
        a64.brute_keep(name)
    return a64.model


def tracer(scene):
    return lambda rays, max_hits, mode, hits: scene.trace_all(rays, max_hits=max_hits, mode=mode, hits=hits)


def lister(scene):
    return lambda rays, mode: scene.trace_lists(rays, mode=mode)


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


class Guarded:
    """A device buffer of `n` elements between two guard regions of PAD elements."""

    def __init__(self, n, dtype, width=None):
        import torch
        shape = (n + 2 * PAD,) if width is None else (n + 2 * PAD, width)
        self.n, self.t = n, torch.full(shape, GUARD, dtype=dtype, device="cuda")
        self.body = self.t[PAD:PAD + n]

    def ptr(self):
        return self.body.data_ptr() if self.n else self.t[PAD:].data_ptr()

    def guards_intact(self):
        a = self.t.cpu().numpy()
        return bool((a[:PAD] == GUARD).all() and (a[PAD + self.n:] == GUARD).all())

    def numpy(self):
        return self.body.cpu().numpy()


def device_flow(gpu, sc, d_rays, n, mode, stream, capacity=None, offsets=None):
    """The documented flow on `stream`: count-only query, scan, read the total, fill; every buffer between
    guards.  offsets: use these instead of the scan's.  Returns (offsets, Guarded hits, Guarded counters, all
    the Guarded buffers)."""
    import torch
    s = stream.cuda_stream
    nbytes = gpu.hit_offsets_scratch_bytes(n)
    with torch.cuda.stream(stream):
        cnt = Guarded(n, torch.int32)
        off = Guarded(n + 1, torch.int64)
        scr = Guarded(nbytes // 8, torch.int64)
        ctr = Guarded(8, torch.int64)
        sc.trace_all_device(d_rays.data_ptr(), n, mode=mode, d_counts=cnt.ptr(), stream=s)
        sc.hit_offsets_device(cnt.ptr(), n, off.ptr(), scr.ptr(), nbytes, stream=s)
        stream.synchronize()
        got_off = off.numpy().view(np.uint64)
        assert np.array_equal(got_off, a64.offsets_of(cnt.numpy().view(np.uint32)))
        if offsets is not None:
            off.body.copy_(torch.from_numpy(offsets.view(np.int64).copy()).cuda())
            got_off = offsets
        total = int(got_off[n])
        hits = Guarded(total, torch.int64, 4)                         # a hit32 record: 4 x 8 B
        sc.trace_lists_device(d_rays.data_ptr(), n, off.ptr(), hits.ptr(), total if capacity is None else capacity, mode=mode,
                              d_counters=ctr.ptr(), stream=s)
    return got_off, hits, ctr, (cnt, off, scr, ctr, hits)


def finish(gpu, hits, ctr, bufs):
    import torch
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in bufs)
    return np.ascontiguousarray(hits.numpy()).view(gpu.HIT64_DTYPE).reshape(-1), ctr.numpy().view(np.uint64)


@pytest.mark.parametrize("name,variant", [(n, v) for n in a64.MODEL_SETS for v in a64.VARIANTS] + [(a64.NANBOX64, "exact_fast")])
def test_gpu_equals_the_model(gpu, scenes, models, name, variant):
    """Counts, rows, prefixes, count-only and the complete lists, bit for bit, on a production and a stats scene;
    on the stats scene node_pairs and tri_tests.  The NaN-leaf soup (an inverted box) in the exact variant."""
    for stats in (False, True):
        sc = scenes(name, variant, stats)
        a64.check_against_model(gpu, tracer(sc), name, variant, stats=stats)
        a64.check_lists_against_model(gpu, lister(sc), name, variant, stats=stats)


@pytest.mark.parametrize("variant", a64.VARIANTS)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_against_the_reference_traversers_answers(gpu, scenes, name, variant):
    a64.check_against_reference_answers(gpu, tracer(scenes(name, variant)), name, variant)


@pytest.mark.parametrize("name", t64.BRUTE_SCENES)
def test_against_brute_force(gpu, scenes, models, name):
    a64.check_against_brute_force(tracer(scenes(name)), name)


@pytest.mark.parametrize("variant", a64.VARIANTS)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_list_properties(gpu, scenes, name, variant):
    mode = t64.variant_mode(gpu, variant)[0]
    rays = t64.load_ray_fixture64(name)["rays"]
    sc = scenes(name, variant)
    counts, _ = a64.check_list_properties(tracer(sc), rays, mode)
    assert (counts == 0).any() and (counts >= 1).any(), name
    a64.check_lists_against_trace_all(lister(sc), tracer(sc), rays, mode)


@pytest.mark.parametrize("hook", [dict(), dict(CERES_DEBUG_LIST_ENTRIES=1, CERES_DEBUG_LIST_SORT_CAP=2), dict(CERES_DEBUG_LIST_SORT_CAP=64),
                                  dict(CERES_DEBUG_LIST_ENTRIES=32)],
                         ids=lambda h: "-".join("%s=%s" % (k[12:], v) for k, v in h.items()) or "default")
def test_rows_past_32_and_long_segments(gpu, models, hook):
    """The dupleaf scene in double: rows of 32 records equal in t; the 130- and 40-record segments through the
    in-LDS sort (default), the in-place sort (sort cap 2 and 64) with 1 list entry, and 32 list entries (the
    40-record segments still past L).  The hooks are read when the scene is created and change no answer."""
    for variant in a64.VARIANTS:
        a64.check_dupleaf_floors(variant)
        for stats in (False, True):
            with env(**hook):
                sc = gpu.Scene(*a64.set_scene(a64.DUPLEAF64, a64.build_of(variant)), stats=stats)
            try:
                a64.check_against_model(gpu, tracer(sc), a64.DUPLEAF64, variant, stats=stats, prefixes=(5,))
                a64.check_lists_against_model(gpu, lister(sc), a64.DUPLEAF64, variant, stats=stats)
            finally:
                sc.close()


@pytest.mark.parametrize("variant", a64.VARIANTS)
def test_gpu_equals_cpu_path(gpu, scenes, variant):
    """All 4,099 rays of dragon_adversarial64 (64 full wavefronts and a tail of 3; NaN, inf and zero
    directions, tmin > tmax): rows at max_hits 1, 8 and 32, the count-only call and the lists, byte for byte."""
    mode = t64.variant_mode(gpu, variant)[0]
    rays = t64.load_ray_fixture64(ADV)["rays"]
    assert len(rays) == 4099 and np.isnan(rays).any() and np.isinf(rays).any()
    sc, cpu = scenes(ADV, variant), scenes.cpu(ADV, variant)
    for K in (1, 8, 32, 0):
        c, r, st = sc.trace_all(rays, max_hits=K, mode=mode, hits=K > 0)
        ec, er, est = cpu.trace_all(rays, max_hits=K, mode=mode, hits=K > 0)
        assert np.array_equal(c, ec), (K, np.flatnonzero(c != ec)[:8])
        assert (r is None and er is None) if K == 0 else a64.rows_equal(r, er), (K, None if K == 0 else a64.first_bad(r, er))
        assert (st["rays"], st["hits"]) == (est["rays"], est["hits"])
    assert (ec > 4).sum() >= 20 and (ec == 0).sum() > 100
    o, h, st = sc.trace_lists(rays, mode=mode)
    eo, eh, est = cpu.trace_lists(rays, mode=mode)
    assert np.array_equal(o, eo) and a64.rows_equal(h, eh) and (st["rays"], st["hits"]) == (est["rays"], est["hits"])


@pytest.mark.parametrize("n", [63, 64, 65])
def test_device_calls_at_wavefront_tails(gpu, scenes, n):
    """The first n rays of the dupleaf set through the device calls: rows at max_hits 5 and the list flow into
    guarded buffers -- nothing is written outside [0, n x max_hits) records or [0, capacity)."""
    import torch
    m = a64.model(a64.DUPLEAF64)
    rays = a64.set_rays(a64.DUPLEAF64)
    sc = scenes(a64.DUPLEAF64)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    assert (m["count"][:63] > a64.MAX_HITS).any() and (m["count"][:63] == 0).any()
    st = torch.cuda.current_stream().cuda_stream
    K = 5
    cnt, rows, ctr = Guarded(n, torch.int32), Guarded(n * K, torch.int64, 4), Guarded(8, torch.int64)
    sc.trace_all_device(d_rays.data_ptr(), n, max_hits=K, d_counts=cnt.ptr(), d_hits16=rows.ptr(), d_counters=ctr.ptr(), stream=st)
    torch.cuda.synchronize()
    assert cnt.guards_intact() and rows.guards_intact() and ctr.guards_intact()
    got = np.ascontiguousarray(rows.numpy()).view(gpu.HIT64_DTYPE).reshape(n, K)
    assert np.array_equal(cnt.numpy().view(np.uint32), m["count"][:n]) and a64.rows_equal(got, np.ascontiguousarray(a64.rows_of(m, K)[:n]))
    c = ctr.numpy().view(np.uint64)
    assert (c[0], c[1], c[2], c[3], c[6], c[7]) == (n, int((m["count"][:n] >= 1).sum()), n, 0, 0, 0)
    off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream())
    h, c = finish(gpu, hits, ctr, bufs)
    total = int(m["offsets"][n])
    assert np.array_equal(off, m["offsets"][:n + 1]) and a64.rows_equal(h, np.ascontiguousarray(m["hits"][:total]))
    assert (c[0], c[1], c[2], c[3], c[6], c[7]) == (n, int((m["count"][:n] >= 1).sum()), n, total, 0, 0)


def test_capacity_below_the_total(gpu, scenes):
    """A fill call with capacity one short of the total, and with capacities inside and at the start of a long
    segment: nothing at or past `capacity` is written, the segments wholly below it are correct and sorted, the
    cut segment holds records of its own ray (unsorted, not corrupt)."""
    import torch
    m = a64.model(a64.DUPLEAF64)
    rays = a64.set_rays(a64.DUPLEAF64)
    n, total = len(rays), len(m["hits"])
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    sc = scenes(a64.DUPLEAF64)
    long_rays = np.flatnonzero(m["count"] > 100)
    k = int(long_rays[len(long_rays) // 2])
    for cap in (total - 1, int(m["offsets"][k]) + 50, int(m["offsets"][k]), 1):
        off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream(), capacity=cap)
        torch.cuda.synchronize()
        assert (hits.numpy()[cap:] == GUARD).all(), cap
        h, c = finish(gpu, hits, ctr, bufs)
        below = int(np.searchsorted(m["offsets"], cap, side="right")) - 1          # rays 0 .. below - 1 lie wholly below
        end = int(m["offsets"][below])
        assert a64.rows_equal(np.ascontiguousarray(h[:end]), np.ascontiguousarray(m["hits"][:end])), cap
        cut = h[end:cap]                                              # the cut segment: records of that ray's set
        own = m["hits"][end:int(m["offsets"][below + 1])]
        assert set(cut["prim"].tolist()) <= set(own["prim"].tolist()) and len(set(cut["prim"].tolist())) == len(cut), cap
        for rec in cut[:8]:
            assert rec.tobytes() == own[own["prim"] == rec["prim"]][0].tobytes(), cap
        assert c[3] == cap and c[7] == 0 and c[0] == n, (cap, c)
    assert len(long_rays) >= 20 and total >= 130 * len(long_rays)


def test_wrong_offsets_raise_the_mismatch_flag(gpu, scenes):
    """Another ray set's offsets (the same rays reversed) and one segment shortened by a record: the device
    call raises counters[7], writes nothing outside [0, capacity) and leaves the guards intact.  The host call
    maps a raised flag to CERES_EHIP by the rule of the float call; with the offsets it computes itself the flag
    cannot be raised, so the device call is where it is seen, and the host call on the same rays succeeds."""
    import torch
    m = a64.model(a64.DUPLEAF64)
    rays = a64.set_rays(a64.DUPLEAF64)
    n = len(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    a = int(np.flatnonzero(m["count"] > 100)[0])
    short = m["offsets"].copy()
    short[a + 1:] -= np.uint64(1)
    other = a64.offsets_of(m["count"][::-1].copy())
    assert not np.array_equal(other, m["offsets"])
    for cap_hook in ({}, dict(CERES_DEBUG_LIST_SORT_CAP=64)):
        with env(**cap_hook):
            sc = gpu.Scene(*a64.set_scene(a64.DUPLEAF64))
        try:
            for wrong in (short, other):
                off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream(), offsets=wrong)
                h, c = finish(gpu, hits, ctr, bufs)
                assert c[7] == 1 and c[6] == 0
            off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream(), offsets=short)
            h, c = finish(gpu, hits, ctr, bufs)
            end = int(m["offsets"][a])
            assert a64.rows_equal(np.ascontiguousarray(h[:end]), np.ascontiguousarray(m["hits"][:end]))
            o2, h2, _ = sc.trace_lists(rays)                          # the library's own offsets: no flag, no error
            assert np.array_equal(o2, m["offsets"]) and a64.rows_equal(h2, m["hits"])
        finally:
            sc.close()


@pytest.mark.parametrize("name", ["tri1", "quad", "dupleaf"])
def test_scenes_changed_in_place(gpu, name):
    """After Scene.refit(moved) on a double scene, and on Scene.from_device_f64 over a GPU-built double tree of
    the moved mesh: trace_all / trace_lists equal a CpuScene taken through the same step, and the move shows."""
    import torch
    mesh, bvh, moved, _ = rc.moved_scene_inputs(gpu, name, f64=True)
    basis, _, W, H, _ = rc.pose_of(gpu, name, f64=True)
    rays = np.array(gpu.camera_rays64(basis, W, H))
    rays[:, 6] = t64.WINDOW_TMIN[np.arange(len(rays)) % 4]
    sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
    dev = cpu2 = None
    try:
        c0, r0, _ = sc.trace_all(rays, max_hits=32)
        ec, er, _ = cpu.trace_all(rays, max_hits=32)
        assert np.array_equal(c0, ec) and a64.rows_equal(r0, er)
        sc.refit(moved)
        cpu.refit(moved)
        c1, r1, _ = sc.trace_all(rays, max_hits=32)
        ec, er, _ = cpu.trace_all(rays, max_hits=32)
        assert np.array_equal(c1, ec) and a64.rows_equal(r1, er), a64.first_bad(r1, er)
        o1, h1, _ = sc.trace_lists(rays)
        eo, eh, _ = cpu.trace_lists(rays)
        assert np.array_equal(o1, eo) and a64.rows_equal(h1, eh)
        a64.check_lists(rays, o1, h1)
        assert (c1 >= 1).any() and (c1 == 0).any() and not a64.rows_equal(r0, r1)
        if name == "dupleaf":
            assert (c1 > a64.MAX_HITS).any()
        n = len(moved)
        d_tri = torch.from_numpy(moved.tri.reshape(-1).copy()).to("cuda:0")
        d_norm = torch.from_numpy(moved.norm.reshape(-1).copy()).to("cuda:0")
        d_nodes = torch.empty(max(2 * n - 1, 1) * 8, dtype=torch.int64, device="cuda:0")
        d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        nn = gpu.build_bvh_device_f64(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream, 0)
        dev = gpu.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), nn, d_prim.data_ptr(), stream=stream)
        cpu2 = gpu.CpuScene(moved, gpu.build_bvh(moved))
        c2, r2, _ = dev.trace_all(rays, max_hits=32)
        ec, er, _ = cpu2.trace_all(rays, max_hits=32)
        assert np.array_equal(c2, ec) and a64.rows_equal(r2, er), a64.first_bad(r2, er)
        o2, h2, _ = dev.trace_lists(rays)
        eo, eh, _ = cpu2.trace_lists(rays)
        assert np.array_equal(o2, eo) and a64.rows_equal(h2, eh)
        assert (c2 >= 1).any() and not a64.rows_equal(r0, r2)
    finally:
        for s in (sc, cpu, dev, cpu2):
            if s is not None:
                s.close()


def test_refusals_before_any_launch(gpu, scenes):
    """Every argument rule of the four GPU entry points, a float scene handed to them (CERES_EUNSUPPORTED), the
    float-named calls on a double scene; nothing is written by a refused call, and the closest query answers
    identically afterwards."""
    import torch
    sc = scenes(a64.DUPLEAF64)
    m = a64.model(a64.DUPLEAF64)
    rays = np.array(a64.set_rays(a64.DUPLEAF64)[:64])
    before = sc.trace(rays, closest=True, occluded=True)
    d_rays = torch.from_numpy(rays).cuda()
    offs = torch.from_numpy(m["offsets"][:65].view(np.int64).copy()).cuda()
    total = int(m["offsets"][64])
    hits, rows, cnt, ctr = Guarded(total, torch.int64, 4), Guarded(64 * 8, torch.int64, 4), Guarded(64, torch.int32), Guarded(8, torch.int64)
    st = torch.cuda.current_stream().cuda_stream
    good = dict(d_rays32=d_rays.data_ptr(), n_rays=64, d_offsets=offs.data_ptr(), d_hits16=hits.ptr(), capacity=total, d_counters=ctr.ptr(), stream=st)
    for change, status in ((dict(d_rays32=d_rays.data_ptr() + 8), -1), (dict(d_hits16=hits.ptr() + 8), -1), (dict(d_offsets=offs.data_ptr() + 4), -1),
                           (dict(d_offsets=0), -1), (dict(d_hits16=0), -1), (dict(d_rays32=0), -1), (dict(mode=gpu.MODE_PRIMARY), -1),
                           (dict(mode=gpu.MODE_QBVH4), -1), (dict(mode=0x80), -1), (dict(mode=gpu.MODE_ROBUST), -6), (dict(n_rays=1 << 31), -6)):
        with pytest.raises(gpu.CeresError, match="error %d:" % status):
            sc.trace_lists_device(**dict(good, **change))
    good = dict(d_rays32=d_rays.data_ptr(), n_rays=64, max_hits=8, d_counts=cnt.ptr(), d_hits16=rows.ptr(), d_counters=ctr.ptr(), stream=st)
    for change, status in ((dict(d_rays32=d_rays.data_ptr() + 8), -1), (dict(d_hits16=rows.ptr() + 8), -1), (dict(d_counts=cnt.ptr() + 2), -1),
                           (dict(d_counts=0, d_hits16=0), -1), (dict(max_hits=0), -1), (dict(max_hits=33), -1), (dict(d_rays32=0), -1),
                           (dict(mode=gpu.MODE_PRIMARY), -1), (dict(mode=0x80), -1), (dict(mode=gpu.MODE_ROBUST), -6), (dict(n_rays=1 << 31), -6)):
        with pytest.raises(gpu.CeresError, match="error %d:" % status):
            sc.trace_all_device(**dict(good, **change))
    torch.cuda.synchronize()
    for b in (hits, rows, cnt, ctr):
        assert (b.t.cpu().numpy() == GUARD).all()
    L = gpu.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    off = np.zeros(65, np.uint64)
    buf = np.zeros(total, gpu.HIT64_DTYPE)
    hcnt, hrows = np.zeros(64, np.uint32), np.zeros((64, 33), gpu.HIT64_DTYPE)
    tot = ctypes.c_uint64(0)
    lists = lambda h, n, mode, r=rays, b=buf, cap=total: L.ceres_trace_rays_lists_f64(   # noqa: E731
        h, None if r is None else vp(r), n, mode, vp(off), None if b is None else vp(b), cap, ctypes.byref(tot), None)
    every = lambda h, n, mode, K, c=hcnt, b=hrows, r=rays: L.ceres_trace_rays_all_f64(   # noqa: E731
        h, None if r is None else vp(r), n, mode, K, None if c is None else vp(c), None if b is None else vp(b), None)
    for bad in (gpu.MODE_PRIMARY, gpu.MODE_QBVH4, 0x80):
        assert lists(sc._h, 64, bad) == -1 and every(sc._h, 64, bad, 8) == -1, bad
    assert lists(sc._h, 64, gpu.MODE_ROBUST) == -6 and every(sc._h, 64, gpu.MODE_ROBUST, 8) == -6
    assert lists(sc._h, 64, 0, r=None) == -1 and lists(sc._h, 64, 0, b=None, cap=3) == -1 and lists(sc._h, 1 << 31, 0) == -6
    assert lists(None, 64, 0) == -1 and every(None, 64, 0, 8) == -1
    assert every(sc._h, 64, 0, 0) == -1 and every(sc._h, 64, 0, 33) == -1 and every(sc._h, 64, 0, 8, c=None, b=None) == -1
    assert every(sc._h, 64, 0, 8, r=None) == -1 and every(sc._h, 1 << 31, 0, 8) == -6
    fmesh, fbvh, _ = gpu.prepare(gpu.configs.CONFIGS["tri1"])
    f = gpu.Scene(fmesh, fbvh)
    try:
        assert lists(f._h, 64, 0) == -6 and "single precision" in L.ceres_last_error().decode()
        assert every(f._h, 64, 0, 8) == -6 and "single precision" in L.ceres_last_error().decode()
        assert L.ceres_trace_rays_lists_f64_device(f._h, ctypes.c_void_p(256), 64, 0, ctypes.c_void_p(256), ctypes.c_void_p(256), 8, None, None) == -6
        assert L.ceres_trace_rays_all_f64_device(f._h, ctypes.c_void_p(256), 64, 0, 8, ctypes.c_void_p(256), ctypes.c_void_p(256), None, None) == -6
    finally:
        f.close()
    assert L.ceres_trace_rays_all(sc._h, vp(rays), 64, 0, 8, vp(hcnt), vp(hrows), None) == -6 and "float scenes" in L.ceres_last_error().decode()
    assert L.ceres_trace_rays_lists(sc._h, vp(rays), 64, 0, vp(off), vp(buf), total, ctypes.byref(tot), None) == -6
    assert "float scenes" in L.ceres_last_error().decode()
    assert not off.any() and not buf.view(np.uint64).any() and tot.value == 0 and not hcnt.any() and not hrows.view(np.uint64).any()
    stt = gpu._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    off[0], tot.value = 7, 7
    assert L.ceres_trace_rays_lists_f64(sc._h, None, 0, 0, vp(off), None, 0, ctypes.byref(tot), ctypes.byref(stt)) == 0     # n_rays = 0
    assert (stt.rays, stt.hits, stt.node_pairs, stt.tri_tests) == (0, 0, 0, 0) and off[0] == 0 and tot.value == 0
    stt = gpu._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    assert L.ceres_trace_rays_all_f64(sc._h, None, 0, 0, 8, vp(hcnt), vp(hrows), ctypes.byref(stt)) == 0
    assert (stt.rays, stt.hits, stt.node_pairs, stt.tri_tests) == (0, 0, 0, 0)
    assert lists(sc._h, 64, 0, b=None, cap=0) == -3 and tot.value == total         # the capacity protocol
    assert str(total) in L.ceres_last_error().decode() and np.array_equal(off, m["offsets"][:65])
    assert lists(sc._h, 64, 0, cap=total - 1) == -3 and not buf.view(np.uint64).any()
    assert lists(sc._h, 64, 0) == 0 and a64.rows_equal(buf, np.ascontiguousarray(m["hits"][:total]))
    assert every(sc._h, 64, 0, 77, b=None) == 0 and np.array_equal(hcnt, m["count"][:64])   # count-only: max_hits ignored
    names = L.ceres_kernel_names().decode().split(",")
    assert all(k in names for k in ("ceres_trace_all64_k", "ceres_trace_lists64_k", "ceres_sort_lists64_k"))
    after = sc.trace(rays, closest=True, occluded=True)
    assert t64.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
