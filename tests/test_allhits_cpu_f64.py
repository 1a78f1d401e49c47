"""All-hits ray queries and complete hit lists on double scenes, CPU path (ceres_trace_rays_all_cpu_f64,
ceres_trace_rays_lists_cpu_f64, CpuScene.trace_all / trace_lists on a double scene): every hit in a ray's
window, in order -- what the reference's traverser.traverse(ray, intersector) presents, with Scalar = double,
to an intersector that never lowers ray.tmax.

The reference harness has no all-hits mode in double, so the pins are: a float64 transcription of the walk
(allhits64_common.model) on four ray sets in both variants, bit for bit in counts, rows, lists and counters;
the reference's stored closest answers of tests/golden/rays64/ through what a never-shrinking window implies
for them; a brute force over all triangles; the properties of sorted lists; leaves of 130 and 40 coincident
triangles; a soup with a leaf that is NaN on one axis (an inverted box); and the refusals.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import allhits64_common as a64
import trace64_common as t64

EINVAL, ENOMEM, EUNSUPPORTED = -1, -3, -6


@pytest.fixture(scope="module")
def scenes(pkg):
    """get(set, variant) -> the CpuScene of a set's double scene prepared for the variant."""
    cache = {}

    def get(name, variant="exact_fast"):
        key = (name, a64.build_of(variant))
        if key not in cache:
            cache[key] = pkg.CpuScene(*a64.set_scene(name, key[1]))
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


def tracer(scene, **kw):
    return lambda rays, max_hits, mode, hits: scene.trace_all(rays, max_hits=max_hits, mode=mode, hits=hits, **kw)


def lister(scene, **kw):
    return lambda rays, mode: scene.trace_lists(rays, mode=mode, **kw)


def test_the_models_fma_is_the_exact_one():
    """allhits64_common.fma / fma_np against the exact rational on operands that cancel and that do not."""
    rng = np.random.default_rng(20261030)
    a = rng.normal(size=4000) * np.exp2(rng.integers(-30, 31, 4000))
    b = rng.normal(size=4000) * np.exp2(rng.integers(-30, 31, 4000))
    c = np.where(rng.integers(0, 2, 4000) == 1, -a * b * (1 + rng.normal(size=4000) * np.exp2(-rng.integers(1, 60, 4000).astype(float))),
                 rng.normal(size=4000) * np.exp2(rng.integers(-60, 61, 4000)))
    exact = np.asarray([t64.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert t64.same_bits(a64.fma_np(a, b, c), exact)
    assert t64.same_bits(np.asarray([a64.fma(x, y, z) for x, y, z in zip(a, b, c)]), exact)
    assert (exact != a * b + c).sum() > 400                           # the single rounding shows
    for x, y, z, e in ((0.0, 5.0, -0.0, 0.0), (-0.0, 5.0, -0.0, -0.0), (np.inf, 1.0, 1.0, np.inf), (1e300, 1e300, -np.inf, -np.inf),
                       (1e300, 1e10, -1e308, np.inf), (1e300, 1.5e8, -1.4e308, t64.fma(1e300, 1.5e8, -1.4e308)), (1e-300, 1e-300, 1.0, 1.0)):
        assert t64.same_bits(a64.fma(x, y, z), e) and t64.same_bits(a64.fma_np(x, y, z), e), (x, y, z)
    assert np.isnan(a64.fma(np.inf, 0.0, 1.0)) and np.isnan(a64.fma_np(np.nan, 1.0, 1.0))


@pytest.mark.parametrize("variant", a64.VARIANTS)
@pytest.mark.parametrize("name", list(a64.MODEL_SETS))
def test_cpu_path_equals_the_model(pkg, scenes, name, variant):
    """Counts, rows at max_hits = 32, prefixes, count-only, the complete lists, node_pairs and tri_tests."""
    sc = scenes(name, variant)
    a64.check_against_model(pkg, tracer(sc), name, variant, stats=True)
    a64.check_lists_against_model(pkg, lister(sc), name, variant, stats=True)


def test_model_floors():
    """What keeps the model comparison from passing vacuously, from the model alone."""
    for name in a64.MODEL_SETS:
        c = a64.model(name)["count"]
        assert (c >= 1).any() and (c == 0).any(), name
    m = a64.model(t64.LATTICE64)
    c, rows = m["count"], a64.rows_of(m)
    assert (c > 16).sum() >= 10 and (c > 8).sum() >= 50
    pair = np.arange(1, a64.MAX_HITS)[None, :] < np.minimum(c, a64.MAX_HITS)[:, None]
    tied = ((rows["t"][:, :-1] == rows["t"][:, 1:]) & pair).any(axis=1)
    assert tied.sum() >= 500, int(tied.sum())                         # tie order is decided by prim
    neg0 = (m["hits"]["t"] == 0) & np.signbit(m["hits"]["t"])
    assert neg0.any() and ((m["hits"]["t"] == 0) & ~np.signbit(m["hits"]["t"])).any()   # -0 and +0 both occur as t
    differ = sum(int((a64.model(n, "exact_fast")["count"] != a64.model(n, "ref_fast")["count"]).sum()) +
                 int(a64.model(n, "exact_fast")["hits"].tobytes() != a64.model(n, "ref_fast")["hits"].tobytes()) for n in a64.MODEL_SETS)
    assert differ > 0                                                 # the variants differ in substance


@pytest.mark.parametrize("variant", a64.VARIANTS)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_against_the_reference_traversers_answers(pkg, scenes, name, variant):
    a64.check_against_reference_answers(pkg, tracer(scenes(name, variant)), name, variant)


@pytest.mark.parametrize("name", t64.BRUTE_SCENES)
def test_against_brute_force(pkg, scenes, name):
    a64.check_against_brute_force(tracer(scenes(name)), name)


def test_the_walk_is_not_a_brute_force():
    """On lattice_ties64, from the model alone: at least 5 rays where the brute force accepts a triangle the
    walk does not."""
    brute, walked = a64.brute_accepted(t64.LATTICE64), a64.model_sets(t64.LATTICE64)
    assert not (walked & ~brute).any()
    assert (brute & ~walked).any(axis=1).sum() >= 5, int((brute & ~walked).any(axis=1).sum())


@pytest.mark.parametrize("variant", a64.VARIANTS)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_list_properties(pkg, scenes, name, variant):
    mode = t64.variant_mode(pkg, variant)[0]
    rays = t64.load_ray_fixture64(name)["rays"]
    sc = scenes(name, variant)
    counts, _ = a64.check_list_properties(tracer(sc), rays, mode)
    assert (counts == 0).any() and (counts >= 1).any(), name
    a64.check_lists_against_trace_all(lister(sc), tracer(sc), rays, mode)


@pytest.mark.parametrize("variant", a64.VARIANTS)
def test_rows_past_32_and_long_segments(pkg, scenes, variant):
    """The dupleaf scene in double (leaves of 130 and 40 coincident triangles): rows of 32 records equal in
    t, ordered and evicted by original index alone; complete lists equal to the model's full sets."""
    a64.check_dupleaf_floors(variant)
    sc = scenes(a64.DUPLEAF64, variant)
    a64.check_against_model(pkg, tracer(sc), a64.DUPLEAF64, variant, stats=True)
    a64.check_lists_against_model(pkg, lister(sc), a64.DUPLEAF64, variant, stats=True)
    a64.check_lists_against_trace_all(lister(sc), tracer(sc), a64.set_rays(a64.DUPLEAF64), t64.variant_mode(pkg, variant)[0])


def test_a_leaf_that_is_nan_on_one_axis(pkg, scenes):
    """A double soup with a leaf whose triangles are all NaN on x keeps an inverted box there: a miss to the
    octant-picked bounds, whatever the ray.  Counts, rows and tri_tests equal the model's; the model's tests
    would be higher with the min / max-of-fmas box test (asserted from the model: rays whose slabs on y and z
    reach such a leaf exist)."""
    _, bvh, rays = a64.nanbox64()
    inv = a64.inverted_leaves(bvh)
    assert len(inv) >= 1
    _, count, first = a64.node_fields(bvh.nodes)
    sc = scenes(a64.NANBOX64)
    a64.check_against_model(pkg, tracer(sc), a64.NANBOX64, "exact_fast", stats=True)
    a64.check_lists_against_model(pkg, lister(sc), a64.NANBOX64, "exact_fast", stats=True)
    m = a64.model(a64.NANBOX64)
    assert (m["count"] >= 1).sum() >= 50 and (m["count"] == 0).any()
    # the same walk with the inverted axis ignored reaches those leaves: the octant-free form would test them
    flipped = bvh.nodes.copy()
    fb = flipped[:, :6].view(np.float64)
    for k in inv:
        bad = fb[k, 0::2] > fb[k, 1::2]
        fb[k, 0::2][bad], fb[k, 1::2][bad] = -np.inf, np.inf
    b2 = [[float(x) for x in row] for row in fb]
    extra = 0
    for k in range(0, len(rays), 4):                                  # the rays aimed at the NaN triangles' cell
        leaves, _ = a64.walk(b2, [int(x) for x in count], [int(x) for x in first], rays[k])
        extra += sum(int(count[n]) for n in leaves if n in set(inv.tolist()))
    assert extra >= 8, extra


def test_threads_do_not_change_the_answer(pkg, scenes):
    rays = t64.load_ray_fixture64("dragon_adversarial64")["rays"]
    sc = scenes("dragon_adversarial64")
    c1, r1, s1 = sc.trace_all(rays, max_hits=8, threads=1)
    c8, r8, s8 = sc.trace_all(rays, max_hits=8, threads=8)
    assert np.array_equal(c1, c8) and a64.rows_equal(r1, r8)
    assert (s1["node_pairs"], s1["tri_tests"], s1["hits"]) == (s8["node_pairs"], s8["tri_tests"], s8["hits"])
    o1, h1, _ = sc.trace_lists(rays, threads=1)
    o8, h8, _ = sc.trace_lists(rays, threads=8)
    assert np.array_equal(o1, o8) and a64.rows_equal(h1, h8)


def test_refusals(pkg, scenes):
    """Each argument rule of the two CPU entry points returns its status and writes nothing, a float scene is
    CERES_EUNSUPPORTED, and the scene answers a closest query identically afterwards."""
    sc = scenes("dragon_adversarial64")
    rays = np.ascontiguousarray(t64.load_ray_fixture64("dragon_adversarial64")["rays"][:64])
    before = sc.trace(rays, closest=True, occluded=True)
    L = pkg.lib()
    for sym in ("ceres_trace_rays_all_cpu_f64", "ceres_trace_rays_lists_cpu_f64", "ceres_trace_rays_all_f64", "ceres_trace_rays_lists_f64",
                "ceres_trace_rays_all_f64_device", "ceres_trace_rays_lists_f64_device"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    cnt = np.zeros(64, np.uint32)
    rows = np.zeros((64, 33), pkg.HIT64_DTYPE)
    call = lambda n, mode, K, c, h: L.ceres_trace_rays_all_cpu_f64(sc._h, vp(rays), n, mode, K, c, h, None, 0)   # noqa: E731
    assert call(64, 0, 0, vp(cnt), vp(rows)) == EINVAL                # a hit buffer with max_hits = 0
    assert call(64, 0, 33, vp(cnt), vp(rows)) == EINVAL               # max_hits > CERES_MAX_HITS
    assert call(64, 0, 8, None, None) == EINVAL                       # neither output
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY, 0x80):
        assert call(64, bad, 8, vp(cnt), vp(rows)) == EINVAL, bad
    assert call(64, pkg.MODE_ROBUST, 8, vp(cnt), vp(rows)) == EUNSUPPORTED      # no robust intersector in double
    assert call(1 << 31, 0, 8, vp(cnt), vp(rows)) == EUNSUPPORTED
    assert L.ceres_trace_rays_all_cpu_f64(sc._h, None, 64, 0, 8, vp(cnt), vp(rows), None, 0) == EINVAL   # null rays
    assert L.ceres_trace_rays_all_cpu_f64(None, vp(rays), 64, 0, 8, vp(cnt), vp(rows), None, 0) == EINVAL
    off = np.zeros(65, np.uint64)
    tot = ctypes.c_uint64(0)
    lists = lambda n, mode, h, cap, r=rays: L.ceres_trace_rays_lists_cpu_f64(   # noqa: E731
        sc._h, None if r is None else vp(r), n, mode, vp(off), h, cap, ctypes.byref(tot), None, 0)
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, 0x80):
        assert lists(64, bad, vp(rows), 64) == EINVAL, bad
    assert lists(64, pkg.MODE_ROBUST, vp(rows), 64) == EUNSUPPORTED
    assert lists(64, 0, None, 3) == EINVAL and lists(1 << 31, 0, vp(rows), 64) == EUNSUPPORTED and lists(64, 0, vp(rows), 64, r=None) == EINVAL
    fmesh, fbvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"])
    f = pkg.CpuScene(fmesh, fbvh)
    try:
        assert L.ceres_trace_rays_all_cpu_f64(f._h, vp(rays), 64, 0, 8, vp(cnt), vp(rows), None, 0) == EUNSUPPORTED
        assert "single precision" in L.ceres_last_error().decode()
        assert L.ceres_trace_rays_lists_cpu_f64(f._h, vp(rays), 64, 0, vp(off), vp(rows), 64, ctypes.byref(tot), None, 0) == EUNSUPPORTED
    finally:
        f.close()
    assert not cnt.any() and not rows.view(np.uint64).any() and not off.any() and tot.value == 0   # nothing was written
    assert L.ceres_trace_rays_all_cpu(sc._h, vp(rays), 64, 0, 8, vp(cnt), vp(rows), None, 0) == EUNSUPPORTED   # the float-named calls
    assert "float scenes" in L.ceres_last_error().decode()
    assert L.ceres_trace_rays_lists_cpu(sc._h, vp(rays), 64, 0, vp(off), vp(rows), 64, ctypes.byref(tot), None, 0) == EUNSUPPORTED
    assert "float scenes" in L.ceres_last_error().decode()
    assert call(64, 0, 77, vp(cnt), None) == 0                        # count-only: max_hits ignored
    assert np.array_equal(cnt, sc.trace_all(rays, max_hits=1)[0])
    for kw in (dict(max_hits=0), dict(max_hits=33), dict(mode=pkg.MODE_PRIMARY), dict(mode=pkg.MODE_ROBUST)):
        with pytest.raises(pkg.CeresError):
            sc.trace_all(rays, **kw)
    with pytest.raises(pkg.CeresError):
        sc.trace_all(np.zeros((3, 7)))
    st = pkg._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    assert L.ceres_trace_rays_all_cpu_f64(sc._h, None, 0, 0, 8, vp(cnt), vp(rows), ctypes.byref(st), 0) == 0   # n_rays = 0
    assert (st.rays, st.hits, st.node_pairs, st.tri_tests) == (0, 0, 0, 0)
    st = pkg._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    off[0], tot.value = 7, 7
    assert L.ceres_trace_rays_lists_cpu_f64(sc._h, None, 0, 0, vp(off), None, 0, ctypes.byref(tot), ctypes.byref(st), 0) == 0
    assert (st.rays, st.hits, st.node_pairs, st.tri_tests) == (0, 0, 0, 0) and off[0] == 0 and tot.value == 0
    c0, r0, s0 = sc.trace_all(np.zeros((0, 8)), max_hits=4)
    assert c0.shape == (0,) and r0.shape == (0, 4) and r0.dtype == pkg.HIT64_DTYPE and s0["rays"] == 0
    eo, eh, _ = sc.trace_lists(rays)                                  # the capacity protocol
    total = len(eh)
    buf = np.zeros(total, pkg.HIT64_DTYPE)
    assert total > 0 and lists(64, 0, None, 0) == ENOMEM and tot.value == total and np.array_equal(off, eo)
    assert str(total) in L.ceres_last_error().decode()
    assert lists(64, 0, vp(buf), total - 1) == ENOMEM and not buf.view(np.uint64).any()
    assert lists(64, 0, vp(buf), total) == 0 and a64.rows_equal(buf, eh)
    names = L.ceres_kernel_names().decode().split(",")
    assert all(k in names for k in ("ceres_trace_all64_k", "ceres_trace_lists64_k", "ceres_sort_lists64_k"))
    after = sc.trace(rays, closest=True, occluded=True)
    assert t64.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
