"""Complete hit lists on the GPU (ceres_trace_lists_k, ceres_sort_lists_k and the 64-bit scan behind
ceres_trace_rays_lists / _device and ceres_hit_offsets_device, Scene.trace_lists, `./render --rays
--hit-lists-out --offsets-out`): every hit of every ray without the 32-record cap, as offsets and records.

Two bars, as for the capped query.  The reference's own complete lists (tests/golden/rays_lists/), compared
directly in the four variants on production and stats scenes; and the CPU path (ceres_trace_rays_lists_cpu,
pinned to the same files by tests/test_hitlists_cpu.py) on every set of allhits_common.ALL_SETS.  Then what
only the GPU has: the three stack widths, the LDS list length and the out-of-LDS sort (test hooks read at scene
creation), the device calls with guard regions on two streams, the scan, wrong offsets, a capacity below the
total, the refusals, scenes changed in place, and the CLI."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import allhits_common as ac
import hitlists_common as hc
import refit_common as rc
import trace_common as tc

pytestmark = pytest.mark.gpu

GUARD = 0x5a5a5a5a
PAD = 64                                                              # guard elements on either side of a buffer


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

    class Get:
        def __call__(self, name, arith=0, stats=False):
            key = (ac.scene_key(name), arith, stats)
            if key not in cache:
                cache[key] = gpu.Scene(*ac.all_set_scene(name, arith), stats=stats)
            return cache[key]

        def cpu(self, name, arith=0):
            key = (ac.scene_key(name), arith, "cpu")
            if key not in cache:
                cache[key] = gpu.CpuScene(*ac.all_set_scene(name, arith))
            return cache[key]

    yield Get()
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def expected(scenes):
    """get(set, mode, arith) -> the CPU path's (offsets, hits, stats) on the set's rays_all rays, computed once."""
    cache = {}

    def get(name, mode, arith):
        key = (name, mode, arith)
        if key not in cache:
            cache[key] = scenes.cpu(name, arith).trace_lists(ac.load_all_fixture(name)["rays"], mode=mode)
        return cache[key]

    return get


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


def assert_same(got, exp, where):
    (o, h), (eo, eh) = got, exp
    assert np.array_equal(o, eo), (where, "offsets: first differing ray", np.flatnonzero(o != eo)[:8])
    assert hc.hits_equal(h, eh), (where, "first differing ray", hc.first_bad_ray(eo, h, eh))


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
    """The documented flow on `stream` (a torch stream): count-only query, scan, read the total, fill.  Every
    buffer sits between guards.  offsets: use these instead of the scan's (wrong-offset tests).  Returns
    (offsets u64 [n + 1], hits HIT_DTYPE [total], counters u64 [8], the Guarded buffers)."""
    import torch
    s = stream.cuda_stream
    nbytes = gpu.hit_offsets_scratch_bytes(n)
    assert nbytes % 8 == 0
    with torch.cuda.stream(stream):                                   # the buffers are filled with guards on this stream too
        cnt = Guarded(n, torch.int32)
        off = Guarded(n + 1, torch.int64)
        scr = Guarded(nbytes // 8, torch.int64)
        ctr = Guarded(8, torch.int64)
        sc.trace_all_device(d_rays.data_ptr(), n, mode=mode, d_counts=cnt.ptr(), stream=s)
        sc.hit_offsets_device(cnt.ptr(), n, off.ptr(), scr.ptr(), nbytes, stream=s)
        stream.synchronize()
        counts = cnt.numpy().view(np.uint32)
        got_off = off.numpy().view(np.uint64)
        assert np.array_equal(got_off, hc.offsets_of(counts))          # the scan against numpy's cumsum
        if offsets is not None:
            off.body.copy_(torch.from_numpy(offsets.view(np.int64)).cuda())
            got_off = offsets
        total = int(got_off[n])
        hits = Guarded(total, torch.int32, 4)
        sc.trace_lists_device(d_rays.data_ptr(), n, off.ptr(), hits.ptr(), total if capacity is None else capacity, mode=mode,
                              d_counters=ctr.ptr(), stream=s)
    return got_off, hits, ctr, (cnt, off, scr, ctr, hits)


def finish(gpu, hits, ctr, bufs):
    import torch
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in bufs)
    return np.ascontiguousarray(hits.numpy()).view(gpu.HIT_DTYPE).reshape(-1), ctr.numpy().view(np.uint64)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", list(hc.LIST_SETS))
def test_gpu_lists_equal_the_reference_traversers_complete_lists(gpu, scenes, name, variant):
    """Against tests/golden/rays_lists/ directly, bit for bit, on a production and a stats scene; on the stats
    scene node_pairs and tri_tests are the reference's summed Statistics."""
    _, arith = tc.variant_mode(gpu, variant)
    for stats in (False, True):
        hc.check_against_list_fixture(gpu, lister(scenes(name, arith, stats)), name, variant, stats=stats)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", [ac.DUPLEAF, "arms6_centroids"])
def test_fill_call_counts_the_walks_it_ran(gpu, scenes, name, variant):
    """d_counters of a device fill call on a stats scene: rays, rays with a non-empty segment, records
    written, and node_pairs / tri_tests equal to the reference's Statistics summed over the rays that have a
    hit -- the others are not walked.  No flag is raised."""
    import torch
    mode, arith = tc.variant_mode(gpu, variant)
    fx = hc.load_list_fixture(name)
    ref = fx[variant]
    sel = ~np.isnan(fx["rays"]).any(axis=1)                           # (the Statistics of a NaN ray: a call of its own, as elsewhere)
    count, steps, tests = ref["count"][sel], ref["steps"][sel], ref["tests"][sel]
    exp = ref["hits"][np.repeat(sel, ref["count"].astype(np.int64))]
    d_rays = torch.from_numpy(np.ascontiguousarray(fx["rays"][sel])).cuda()
    n = int(sel.sum())
    off, hits, ctr, bufs = device_flow(gpu, scenes(name, arith, True), d_rays, n, mode, torch.cuda.Stream())
    h, c = finish(gpu, hits, ctr, bufs)
    assert np.array_equal(off, hc.offsets_of(count)) and hc.hits_equal(h, np.ascontiguousarray(exp))
    walked = count > 0
    assert 0 < walked.sum() < n
    assert (c[0], c[1], c[2], c[3]) == (n, int(walked.sum()), n, len(exp))
    assert c[4] == int(steps[walked].sum(dtype=np.uint64)) and c[5] == int(tests[walked].sum(dtype=np.uint64))
    assert c[6] == 0 and c[7] == 0


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", ac.ALL_SETS)
def test_gpu_equals_cpu_path(gpu, scenes, expected, name, variant):
    """Offsets and records bit for bit on every set, in the four modes."""
    mode, arith = tc.variant_mode(gpu, variant)
    eo, eh, est = expected(name, mode, arith)
    o, h, st = scenes(name, arith).trace_lists(ac.load_all_fixture(name)["rays"], mode=mode)
    assert_same((o, h), (eo, eh), (name, variant))
    assert (st["rays"], st["hits"]) == (est["rays"], est["hits"])


@pytest.mark.parametrize("hook", [dict(CERES_DEBUG_STACK_WIDTH=3), dict(CERES_DEBUG_STACK_WIDTH=4), dict(CERES_DEBUG_LIST_SORT_CAP=64),
                                  dict(CERES_DEBUG_LIST_ENTRIES=1), dict(CERES_DEBUG_LIST_ENTRIES=32),
                                  dict(CERES_DEBUG_STACK_WIDTH=4, CERES_DEBUG_LIST_SORT_CAP=2, CERES_DEBUG_LIST_ENTRIES=3)],
                         ids=lambda h: "-".join("%s=%s" % (k[12:], v) for k, v in h.items()))
@pytest.mark.parametrize("name", [ac.DUPLEAF, hc.SOUP_LONG])
def test_hooks_change_no_answer(gpu, name, hook):
    """dupleaf_stack (170 hits of two t) and the soup subset (987 hits) at the 24- and 32-bit stack widths, with
    the LDS sort cap lowered so that the in-place sort in global memory runs, and with 1 and 32 LDS list
    entries: the stored reference lists, bit for bit."""
    for variant in ("exact_fast", "ref_robust"):
        _, arith = tc.variant_mode(gpu, variant)
        for stats in (False, True):
            with env(**hook):
                sc = gpu.Scene(*ac.all_set_scene(name, arith), stats=stats)
            try:
                if "CERES_DEBUG_STACK_WIDTH" in hook:
                    assert sc.stack_width() == hook["CERES_DEBUG_STACK_WIDTH"]
                hc.check_against_list_fixture(gpu, lister(sc), name, variant, stats=stats)
            finally:
                sc.close()


def test_device_calls_at_wavefront_tails_on_two_streams(gpu, scenes):
    """The first 63, 64 and 65 rays of dupleaf_stack through the device flow, two flows of one scene in flight
    on two streams with their own buffers and counters: the stored lists; the scan equals numpy's cumsum
    (device_flow); the guard regions around counts, offsets, scratch, counters and records are untouched."""
    import torch
    fx = hc.load_list_fixture(ac.DUPLEAF)
    ref = fx["exact_fast"]
    sc = scenes(ac.DUPLEAF)
    d_rays = torch.from_numpy(np.array(fx["rays"])).cuda()
    assert (ref["count"][:63] > ac.MAX_HITS).any() and (ref["count"][:63] == 0).any()
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    for n, m in ((63, 65), (64, 320)):
        a = device_flow(gpu, sc, d_rays, n, 0, s0)
        b = device_flow(gpu, sc, d_rays, m, 0, s1)
        for k, (off, hits, ctr, bufs) in ((n, a), (m, b)):
            h, c = finish(gpu, hits, ctr, bufs)
            total = int(ref["offsets"][k])
            assert np.array_equal(off, ref["offsets"][:k + 1]), k
            assert hc.hits_equal(h, np.ascontiguousarray(ref["hits"][:total])), k
            assert (c[0], c[1], c[2], c[3], c[6], c[7]) == (k, int((ref["count"][:k] >= 1).sum()), k, total, 0, 0), k


def test_scan_scratch_is_the_callers(gpu, scenes):
    """ceres_hit_offsets_scratch_bytes is honoured (one byte less: CERES_EINVAL, nothing written); counts past
    one scan block and sums past 2^32."""
    import torch
    sc = scenes(ac.DUPLEAF)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(20261101)
    for n in (1, 1023, 1024, 1025, 70001):
        counts = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if n == 70001 else rng.integers(0, 9, n).astype(np.uint32)
        cnt = Guarded(n, torch.int32)
        cnt.body.copy_(torch.from_numpy(counts.view(np.int32)).cuda())
        off = Guarded(n + 1, torch.int64)
        nbytes = gpu.hit_offsets_scratch_bytes(n)
        scr = Guarded(nbytes // 8, torch.int64)
        with pytest.raises(gpu.CeresError, match="error -1"):
            sc.hit_offsets_device(cnt.ptr(), n, off.ptr(), scr.ptr(), nbytes - 1, stream=st)
        with pytest.raises(gpu.CeresError, match="error -1"):
            sc.hit_offsets_device(cnt.ptr(), n, off.ptr() + 4, scr.ptr(), nbytes, stream=st)
        torch.cuda.synchronize()
        assert (off.numpy() == GUARD).all()
        sc.hit_offsets_device(cnt.ptr(), n, off.ptr(), scr.ptr(), nbytes, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(off.numpy().view(np.uint64), hc.offsets_of(counts)), n
        assert off.guards_intact() and scr.guards_intact() and cnt.guards_intact(), n
    assert int(hc.offsets_of(counts)[-1]) > 1 << 40


def test_wrong_offsets_raise_the_mismatch_flag(gpu, scenes):
    """One long ray's segment shortened by one record and a later one's lengthened by one (wrong arguments;
    the kernel clamps to the segment): the mismatch flag is set, every other ray's segment holds its correct
    records, the guards are intact.  The host call maps a set flag to CERES_EHIP by the documented rule --
    with its own offsets it cannot be set, so the device call is where the flag is seen."""
    import torch
    fx = hc.load_list_fixture(ac.DUPLEAF)
    ref = fx["exact_fast"]
    n = len(fx["rays"])
    long_rays = np.flatnonzero(ref["count"] > 100)
    a, b = int(long_rays[0]), int(long_rays[-1])
    assert a + 1 < b
    wrong = ref["offsets"].copy()
    wrong[a + 1:b + 1] -= np.uint64(1)                                # a: one short; a + 1 .. b - 1: moved; b: one long
    d_rays = torch.from_numpy(np.array(fx["rays"])).cuda()
    for cap_hook in ({}, dict(CERES_DEBUG_LIST_SORT_CAP=64)):
        with env(**cap_hook):
            sc = gpu.Scene(*ac.all_set_scene(ac.DUPLEAF, 0))
        try:
            off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream(), offsets=wrong)
            h, c = finish(gpu, hits, ctr, bufs)
            assert c[7] == 1 and c[6] == 0
            for r in range(n):
                if r not in (a, b):
                    got, exp = h[int(wrong[r]):int(wrong[r + 1])], ref["hits"][int(ref["offsets"][r]):int(ref["offsets"][r + 1])]
                    assert hc.hits_equal(np.ascontiguousarray(got), np.ascontiguousarray(exp)), r
            o2, h2, st = sc.trace_lists(fx["rays"])                    # the library's own offsets: no flag, no error
            assert np.array_equal(o2, ref["offsets"]) and hc.hits_equal(h2, ref["hits"])
        finally:
            sc.close()


def test_capacity_below_the_total(gpu, scenes):
    """The device fill call with capacity < total: nothing at or past `capacity` is written, the segments
    wholly below it are correct; capacity 0 with no buffer writes nothing at all and still counts."""
    import torch
    fx = hc.load_list_fixture(ac.DUPLEAF)
    ref = fx["exact_fast"]
    n = len(fx["rays"])
    total = len(ref["hits"])
    d_rays = torch.from_numpy(np.array(fx["rays"])).cuda()
    sc = scenes(ac.DUPLEAF)
    k = int(np.flatnonzero(ref["count"] > 100)[len(np.flatnonzero(ref["count"] > 100)) // 2])
    for cap in (int(ref["offsets"][k]) + 50, int(ref["offsets"][k]), 1):          # inside a long segment; at its start
        off, hits, ctr, bufs = device_flow(gpu, sc, d_rays, n, 0, torch.cuda.Stream(), capacity=cap)
        torch.cuda.synchronize()
        raw = hits.numpy()
        assert (raw[cap:] == GUARD).all(), cap
        h, c = finish(gpu, hits, ctr, bufs)
        below = int(np.searchsorted(ref["offsets"], cap, side="right")) - 1       # rays 0 .. below - 1 lie wholly below
        end = int(ref["offsets"][below])
        assert hc.hits_equal(np.ascontiguousarray(h[:end]), np.ascontiguousarray(ref["hits"][:end])), cap
        assert c[3] == cap and c[7] == 0 and c[0] == n, (cap, c)
    ctr = Guarded(8, torch.int64)
    offs = torch.from_numpy(ref["offsets"].view(np.int64).copy()).cuda()
    sc.trace_lists_device(d_rays.data_ptr(), n, offs.data_ptr(), 0, 0, d_counters=ctr.ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = ctr.numpy().view(np.uint64)
    assert ctr.guards_intact() and (c[0], c[1], c[3], c[7]) == (n, int((ref["count"] >= 1).sum()), 0, 0)
    assert total > 15000


def test_refusals_before_any_launch(gpu, scenes):
    """Misaligned pointers, bad modes, a null buffer with a capacity, 2^31 rays and a double scene are refused
    with their statuses; nothing is written, and the scene answers a closest query identically afterwards."""
    import torch
    sc = scenes(ac.DUPLEAF)
    fx = hc.load_list_fixture(ac.DUPLEAF)
    rays = np.array(fx["rays"][:64])
    before = sc.trace(rays, closest=True, occluded=True)
    d_rays = torch.from_numpy(rays).cuda()
    offs = torch.from_numpy(fx["exact_fast"]["offsets"][:65].view(np.int64).copy()).cuda()
    total = int(fx["exact_fast"]["offsets"][64])
    hits = Guarded(total, torch.int32, 4)
    ctr = Guarded(8, torch.int64)
    st = torch.cuda.current_stream().cuda_stream
    good = dict(d_rays32=d_rays.data_ptr(), n_rays=64, d_offsets=offs.data_ptr(), d_hits16=hits.ptr(), capacity=total, d_counters=ctr.ptr(), stream=st)
    for change, status in ((dict(d_rays32=d_rays.data_ptr() + 4), -1), (dict(d_hits16=hits.ptr() + 8), -1), (dict(d_offsets=offs.data_ptr() + 4), -1),
                           (dict(d_offsets=0), -1), (dict(d_hits16=0), -1), (dict(d_rays32=0), -1), (dict(mode=gpu.MODE_PRIMARY), -1),
                           (dict(mode=gpu.MODE_QBVH4), -1), (dict(mode=0x80), -1), (dict(n_rays=1 << 31), -6)):
        with pytest.raises(gpu.CeresError, match="error %d:" % status):
            sc.trace_lists_device(**dict(good, **change))
    torch.cuda.synchronize()
    assert (hits.t.cpu().numpy() == GUARD).all() and (ctr.t.cpu().numpy() == GUARD).all()
    L = gpu.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    off = np.zeros(65, np.uint64)
    buf = np.zeros(total, gpu.HIT_DTYPE)
    tot = ctypes.c_uint64(0)
    call = lambda h, n, mode, r=rays, b=buf, cap=total: L.ceres_trace_rays_lists(   # noqa: E731
        h, None if r is None else vp(r), n, mode, vp(off), None if b is None else vp(b), cap, ctypes.byref(tot), None)
    for bad in (gpu.MODE_PRIMARY, gpu.MODE_QBVH4, 0x80):
        assert call(sc._h, 64, bad) == -1, bad
    assert call(sc._h, 64, 0, r=None) == -1 and call(sc._h, 64, 0, b=None, cap=3) == -1 and call(sc._h, 1 << 31, 0) == -6
    assert call(None, 64, 0) == -1
    mesh, bvh, _ = gpu.prepare(gpu.configs.CONFIGS["tri1"], f64=True)
    d = gpu.Scene(mesh, bvh)
    try:
        assert call(d._h, 64, 0) == -6 and "float scenes" in L.ceres_last_error().decode()
        assert L.ceres_trace_rays_lists_device(d._h, ctypes.c_void_p(256), 64, 0, ctypes.c_void_p(256), ctypes.c_void_p(256), 8, None, None) == -6
    finally:
        d.close()
    assert not off.any() and not buf.view(np.uint32).any() and tot.value == 0
    stt = gpu._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    off[0], tot.value = 7, 7
    assert L.ceres_trace_rays_lists(sc._h, None, 0, 0, vp(off), None, 0, ctypes.byref(tot), ctypes.byref(stt)) == 0     # n_rays = 0
    assert (stt.rays, stt.hits, stt.node_pairs, stt.tri_tests) == (0, 0, 0, 0) and off[0] == 0 and tot.value == 0
    assert call(sc._h, 64, 0, b=None, cap=0) == hc.ENOMEM and tot.value == total       # the capacity protocol
    assert str(total) in L.ceres_last_error().decode() and np.array_equal(off, fx["exact_fast"]["offsets"][:65])
    assert call(sc._h, 64, 0, cap=total - 1) == hc.ENOMEM and not buf.view(np.uint32).any()
    assert call(sc._h, 64, 0) == 0 and hc.hits_equal(buf, np.ascontiguousarray(fx["exact_fast"]["hits"][:total]))
    after = sc.trace(rays, closest=True, occluded=True)
    assert tc.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("how", ["refit", "rebuild"])
@pytest.mark.parametrize("name", ["tri1", "dupleaf"])
def test_scenes_changed_in_place(gpu, name, how):
    """trace_lists after Scene.refit(moved) and after Scene.rebuild(moved): equal to a CpuScene taken through
    the same call, and the move shows."""
    mesh, bvh, moved, _ = rc.moved_scene_inputs(gpu, name)
    basis, _, W, H, _ = rc.pose_of(gpu, name)
    rays = np.ascontiguousarray(gpu.camera_rays(basis, W, H))
    rays[:, 6] = tc.WINDOW_TMIN[np.arange(len(rays)) % 4]
    sc, cpu = gpu.Scene(mesh, bvh), gpu.CpuScene(mesh, bvh)
    try:
        o0, h0, _ = sc.trace_lists(rays)
        assert_same((o0, h0), cpu.trace_lists(rays)[:2], (name, "before"))
        getattr(sc, how)(moved)
        getattr(cpu, how)(moved)
        o1, h1, st = sc.trace_lists(rays)
        assert_same((o1, h1), cpu.trace_lists(rays)[:2], (name, how))
        hc.check_lists(rays, o1, h1)
        counts = np.diff(o1.astype(np.int64))
        assert (counts >= 1).any() and (counts == 0).any() and not hc.hits_equal(h0, h1)
        if name == "dupleaf":
            assert (counts > ac.MAX_HITS).any()
    finally:
        sc.close()
        cpu.close()


def test_cli_on_the_gpu(gpu, tmp_path):
    """./render --rays --hit-lists-out --offsets-out: the --cpu run's files, byte for byte."""
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    rf = tmp_path / "rays.bin"
    rf.write_bytes(rays.tobytes())
    out = {}
    for where in ("gpu", "cpu"):
        hf, of = tmp_path / (where + "_lists.bin"), tmp_path / (where + "_offsets.bin")
        args = [gpu.CLI_PATH, tc.LATTICE_OBJ, "--exact", "--rays", str(rf), "--hit-lists-out", str(hf), "--offsets-out", str(of)]
        r = subprocess.run(args + (["--cpu"] if where == "cpu" else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[where] = (hf.read_bytes(), of.read_bytes())
    assert out["gpu"] == out["cpu"] and len(out["gpu"][1]) == (len(rays) + 1) * 8 and len(out["gpu"][0]) > 16 * 1000
    r = subprocess.run([gpu.CLI_PATH, tc.LATTICE_OBJ, "--double", "--rays", str(rf), "--hit-lists-out", str(tmp_path / "x.bin"),
                        "--offsets-out", str(tmp_path / "y.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "float scenes" in r.stderr
