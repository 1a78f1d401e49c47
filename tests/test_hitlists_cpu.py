"""Complete hit lists on the CPU path (ceres_trace_rays_lists_cpu, CpuScene.trace_lists, `./render --cpu
--rays --hit-lists-out --offsets-out`): every hit of every ray without the 32-record cap, as offsets and
records.

The pins: the reference's own complete lists (tests/golden/rays_lists/, its traverser's collecting run stored
whole, four variants) bit for bit with offsets and counters; the capped query CpuScene.trace_all on every set
of allhits_common.ALL_SETS (counts, the first 32 records, strictly increasing keys, windows); the capacity
protocol; the refusals; the CLI.  No GPU needed."""
import ctypes
import subprocess

import numpy as np
import pytest

import allhits_common as ac
import hitlists_common as hc
import trace_common as tc


@pytest.fixture(scope="module")
def all_set_scene(pkg):
    """get(set, arith) -> the CpuScene of any set of ac.ALL_SETS."""
    cache = {}

    def get(name, arith=0):
        key = (ac.scene_key(name), arith)
        if key not in cache:
            cache[key] = pkg.CpuScene(*ac.all_set_scene(name, arith))
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


def lister(scene, **kw):
    return lambda rays, mode: scene.trace_lists(rays, mode=mode, **kw)


def tracer(scene):
    return lambda rays, max_hits, mode, hits: scene.trace_all(rays, max_hits=max_hits, mode=mode, hits=hits)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", list(hc.LIST_SETS))
def test_cpu_lists_equal_the_reference_traversers_complete_lists(pkg, all_set_scene, name, variant):
    """Against tests/golden/rays_lists/: offsets = [0] + cumsum(counts), every record, rays / hits, and
    node_pairs / tri_tests equal to the reference's summed Statistics -- bit for bit."""
    sc = all_set_scene(name, tc.variant_mode(pkg, variant)[1])
    hc.check_against_list_fixture(pkg, lister(sc), name, variant, stats=True)


def test_list_fixture_floors(pkg):
    """The stored lists reach what they are there for, and their heads are the rays_all rows."""
    assert ac.HIT_DTYPE == pkg.HIT_DTYPE
    hc.check_list_fixture_floors()
    for name in hc.LIST_SETS:
        for v in tc.RAY_VARIANTS:
            fx, cap = hc.load_list_fixture(name)[v], ac.load_all_fixture(name)[v]
            n = len(fx["count"])
            assert np.array_equal(fx["count"], cap["count"][:n]), (name, v)
            hc.check_lists(hc.load_list_fixture(name)["rays"], fx["offsets"], fx["hits"])


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", ac.ALL_SETS)
def test_cpu_lists_against_the_capped_query(pkg, all_set_scene, name, variant):
    """On every set: counts equal CpuScene.trace_all's, each list's first min(count, 32) records are its
    max_hits = 32 row, keys strictly increase, every t lies in its ray's window."""
    mode, arith = tc.variant_mode(pkg, variant)
    sc = all_set_scene(name, arith)
    hc.check_against_trace_all(lister(sc), tracer(sc), ac.load_all_fixture(name)["rays"], mode)


def test_threads_do_not_change_the_answer(pkg, all_set_scene):
    rays = hc.list_rays(ac.DUPLEAF)
    sc = all_set_scene(ac.DUPLEAF, 0)
    o1, h1, s1 = sc.trace_lists(rays, threads=1)
    o8, h8, s8 = sc.trace_lists(rays, threads=8)
    assert np.array_equal(o1, o8) and hc.hits_equal(h1, h8)
    assert (s1["node_pairs"], s1["tri_tests"], s1["hits"]) == (s8["node_pairs"], s8["tri_tests"], s8["hits"])


def test_capacity_protocol(pkg, all_set_scene):
    """capacity 0 without a buffer: CERES_ENOMEM with offsets and the total; capacity = total - 1: nothing is
    written anywhere in the buffer; capacity = total: the answer; a set of rays that all miss: total 0 and
    success without a buffer."""
    L = pkg.lib()
    sc = all_set_scene(ac.DUPLEAF, 0)
    rays = hc.list_rays(ac.DUPLEAF)
    n = len(rays)
    ref = hc.load_list_fixture(ac.DUPLEAF)["exact_fast"]
    total_ref = len(ref["hits"])
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731

    def call(off, hits, cap, r=rays):
        total, st = ctypes.c_uint64(99), pkg._Stats()
        rc = L.ceres_trace_rays_lists_cpu(sc._h, vp(r), len(r), 0, None if off is None else vp(off), None if hits is None else vp(hits),
                                          cap, ctypes.byref(total), ctypes.byref(st), 0)
        return rc, total.value, st

    off = np.full(n + 1, 7, np.uint64)
    rc, total, st = call(off, None, 0)
    assert rc == hc.ENOMEM and total == total_ref and np.array_equal(off, ref["offsets"])
    msg = L.ceres_last_error().decode()
    assert str(total_ref) in msg and "capacity 0" in msg, msg
    assert st.rays == n and st.hits == int((ref["count"] >= 1).sum())
    guard = np.full(total_ref + 8, 0xa5a5a5a5, np.uint32).repeat(4).view(pkg.HIT_DTYPE)
    buf = guard.copy()
    off[:] = 7
    rc, total, _ = call(off, buf, total_ref - 1)
    assert rc == hc.ENOMEM and total == total_ref and np.array_equal(off, ref["offsets"])
    assert str(total_ref - 1) in L.ceres_last_error().decode()
    assert hc.hits_equal(buf, guard)                                  # no record was written
    rc, total, _ = call(None, buf, total_ref)                         # offsets may be NULL
    assert rc == 0 and total == total_ref
    assert hc.hits_equal(np.ascontiguousarray(buf[:total_ref]), ref["hits"]) and hc.hits_equal(buf[total_ref:], guard[total_ref:])
    assert L.ceres_trace_rays_lists_cpu(sc._h, vp(rays), n, 0, None, vp(buf), total_ref, None, None, 0) == 0   # total, stats NULL
    miss = np.ascontiguousarray(rays[ref["count"] == 0])
    assert len(miss) >= 8
    off = np.full(len(miss) + 1, 7, np.uint64)
    rc, total, st = call(off, None, 0, miss)
    assert rc == 0 and total == 0 and not off.any() and st.hits == 0 and st.rays == len(miss)
    o, h, st = sc.trace_lists(miss)
    assert h.shape == (0,) and not o.any() and st["hits"] == 0


def test_refusals(pkg, all_set_scene):
    """Each argument rule returns its status, nothing is written, and the scene answers a closest query
    identically afterwards."""
    sc = all_set_scene(ac.DUPLEAF, 0)
    rays = np.ascontiguousarray(hc.list_rays(ac.DUPLEAF)[:64])
    before = sc.trace(rays, closest=True, occluded=True)
    L = pkg.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    off = np.zeros(65, np.uint64)
    buf = np.zeros(4096, pkg.HIT_DTYPE)
    total = ctypes.c_uint64(0)
    call = lambda n, mode, r=rays, h=buf, cap=4096: L.ceres_trace_rays_lists_cpu(   # noqa: E731
        sc._h, None if r is None else vp(r), n, mode, vp(off), None if h is None else vp(h), cap, ctypes.byref(total), None, 0)
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY, 0x80):
        assert call(64, bad) == hc.EINVAL, bad
    assert call(64, 0, r=None) == hc.EINVAL                           # null rays
    assert call(64, 0, h=None, cap=5) == hc.EINVAL                    # no buffer, yet a capacity
    assert call(1 << 31, 0) == hc.EUNSUPPORTED
    assert L.ceres_trace_rays_lists_cpu(None, vp(rays), 64, 0, vp(off), vp(buf), 4096, None, None, 0) == hc.EINVAL
    assert not off.any() and not buf.view(np.uint32).any() and total.value == 0
    with pytest.raises(pkg.CeresError):
        sc.trace_lists(rays, mode=pkg.MODE_PRIMARY)
    with pytest.raises(pkg.CeresError):
        sc.trace_lists(np.zeros((3, 7), np.float32))
    st = pkg._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    off[0], total.value = 7, 7
    assert L.ceres_trace_rays_lists_cpu(sc._h, None, 0, 0, vp(off), None, 0, ctypes.byref(total), ctypes.byref(st), 0) == 0   # n_rays = 0
    assert (st.rays, st.hits, st.node_pairs, st.tri_tests) == (0, 0, 0, 0) and off[0] == 0 and total.value == 0
    o0, h0, s0 = sc.trace_lists(np.zeros((0, 8), np.float32))
    assert o0.shape == (1,) and o0[0] == 0 and h0.shape == (0,) and s0["rays"] == 0
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"], f64=True)
    d = pkg.CpuScene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_lists_cpu(d._h, vp(rays), 64, 0, vp(off), vp(buf), 4096, None, None, 0) == hc.EUNSUPPORTED
        assert "float scenes" in L.ceres_last_error().decode()
    finally:
        d.close()
    names = L.ceres_kernel_names().decode().split(",")
    assert {"ceres_trace_lists_k", "ceres_sort_lists_k", "ceres_scan64_reduce", "ceres_scan64_partials", "ceres_scan64_down"} <= set(names)
    after = sc.trace(rays, closest=True, occluded=True)
    assert tc.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_cli_cpu_hit_lists(pkg, all_set_scene, tmp_path):
    """./render --cpu --rays --hit-lists-out --offsets-out on tests/golden/lattice.obj: the files hold
    CpuScene.trace_lists's bytes; --double: the library's refusal, status 1; one file missing or a
    combination with another ray query's outputs: bad usage, status 2."""
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    cfg = tc.ray_set_config(tc.LATTICE)
    off, hits, st = all_set_scene(tc.LATTICE, 0).trace_lists(rays)
    assert len(hits) > 1000
    rf, hf, of, xf = tmp_path / "rays.bin", tmp_path / "lists.bin", tmp_path / "offsets.bin", tmp_path / "x.bin"
    rf.write_bytes(rays.tobytes())
    base = [pkg.CLI_PATH, tc.LATTICE_OBJ]
    if cfg.get("rotate"):
        base += ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    base += ["--exact", "--cpu", "--rays", str(rf)]
    run = lambda *a: subprocess.run(base + list(a), capture_output=True, text=True, timeout=120)   # noqa: E731
    both = ("--hit-lists-out", str(hf), "--offsets-out", str(of))
    r = run("--json", *both)
    assert r.returncode == 0, r.stderr
    assert hf.read_bytes() == hits.tobytes() and of.read_bytes() == off.tobytes()
    assert '"rays": %d, "hits": %d, "records": %d' % (len(rays), st["hits"], len(hits)) in r.stdout
    r = run("--double", *both)
    assert r.returncode == 1 and "float scenes" in r.stderr
    for bad in (("--hit-lists-out", str(hf)), ("--offsets-out", str(of)), both + ("--all-hits", "5"), both + ("--hits-out", str(xf)),
                both + ("--occluded-out", str(xf)), both + ("--all-hits", "0", "--counts-out", str(xf)),
                both + ("--pixels-out", str(xf)), both + ("--status-out", str(xf))):
        assert run(*bad).returncode == 2, bad
    assert not xf.exists()
