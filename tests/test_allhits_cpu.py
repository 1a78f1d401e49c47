"""All-hits ray queries on the CPU path (ceres_trace_rays_all_cpu, CpuScene.trace_all, `./render --cpu
--rays --all-hits`): every hit in a ray's window, in order -- what the reference's
traverser.traverse(ray, intersector) presents to an intersector that never lowers ray.tmax.

The pins: the reference's own answer -- its traverser run with a collecting intersector whose distance() is
ray.tmax (oracle/ref_harness.cpp --ray-all-hits), stored under tests/golden/rays_all/ for the eight ray sets,
for dupleaf_stack (leaves of 130 and 40 coincident triangles: rows past 32 records equal in t) and for four
non-finite soups, in all four variants -- equal bit for bit in counts, rows, prefixes and counters; a Python
transcription of the walk over the reference-layout nodes (allhits_common.model), equal bit for bit on four
sets in exact_fast; the reference's stored closest answers (tests/golden/rays/), through what a
never-shrinking window implies for them; the properties of a sorted, truncated list; and floors that keep
all of it from passing vacuously.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import allhits_common as ac
import trace_common as tc


@pytest.fixture(scope="module")
def ray_set_scene(pkg):
    """get(set, arith) -> the CpuScene of a ray set's scene."""
    cache = {}

    def get(name, arith=0):
        key = ("proc300" if name == "proc300_window" else tc.ray_set_config(name)["obj"], arith)
        if key not in cache:
            cache[key] = pkg.CpuScene(*tc.ray_set_scene(name, arith))
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


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


def tracer(scene, **kw):
    return lambda rays, max_hits, mode, hits: scene.trace_all(rays, max_hits=max_hits, mode=mode, hits=hits, **kw)


@pytest.fixture(scope="module")
def answers(pkg, ray_set_scene):
    """get(set) -> (counts, rows at max_hits = 32) of the exact_fast variant, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            c, r, _ = ray_set_scene(name, 0).trace_all(tc.load_ray_fixture(name)["rays"], max_hits=ac.MAX_HITS, mode=0)
            cache[name] = (c, r)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(ac.MODEL_SETS))
def test_cpu_path_equals_the_model(pkg, ray_set_scene, name):
    """Counts, records, node_pairs and tri_tests at max_hits = 32, bit for bit (the whole set; the first
    512 rays of dragon_adversarial)."""
    rays = np.ascontiguousarray(tc.load_ray_fixture(name)["rays"][:ac.MODEL_SETS[name]])
    counts, rows, steps, tests = ac.model(name)
    c, r, st = ray_set_scene(name, 0).trace_all(rays, max_hits=ac.MAX_HITS, mode=0)
    assert np.array_equal(c, counts), np.flatnonzero(c != counts)[:8]
    bad = np.flatnonzero((r.view(np.uint32) != rows.view(np.uint32)).reshape(len(rays), -1).any(axis=1))
    assert ac.rows_equal(r, rows), ("first differing ray", bad[:8])
    assert (st["node_pairs"], st["tri_tests"]) == (steps, tests)
    assert st["rays"] == len(rays) and st["hits"] == int((counts >= 1).sum())
    assert (counts >= 1).any() and (counts == 0).any()


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", ac.ALL_SETS)
def test_cpu_path_equals_the_reference_traversers_all_hits(pkg, all_set_scene, name, variant):
    """Against tests/golden/rays_all/: counts and rows at max_hits = 32, the rows of 1 and 5 as prefixes, the
    count-only call, and node_pairs / tri_tests equal to the reference's summed Statistics -- bit for bit."""
    sc = all_set_scene(name, tc.variant_mode(pkg, variant)[1])
    ac.check_against_all_fixture(pkg, tracer(sc), name, variant, stats=True)


def test_all_hits_fixture_floors_and_inputs(pkg):
    """The stored reference answers reach what they are there for (rows past 32, 40 and 130 hits of one t,
    empty rows, soups with several hits, variants that differ); the new sets' stored rays are what their
    generators give today; the dupleaf stacks read from the OBJ text are the package's triangles."""
    assert ac.HIT_DTYPE == pkg.HIT_DTYPE
    ac.check_all_fixture_floors()
    for name in ac.NEW_SETS:
        assert tc.same_bits(ac.load_all_fixture(name)["rays"], ac.new_set_rays(name)), name
    mesh, _ = ac.all_set_scene(ac.DUPLEAF, 0)
    for vertices, copies, first in ac.dupleaf_stacks():
        row = ac._tri_rows(vertices[None])[0]
        same = (mesh.tri.view(np.uint32) == row.view(np.uint32)).all(axis=1)
        assert same.sum() == copies and same[first], copies


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_against_the_reference_traversers_answers(pkg, ray_set_scene, name, variant):
    sc = ray_set_scene(name, tc.variant_mode(pkg, variant)[1])
    ac.check_against_reference_answers(pkg, tracer(sc), name, variant)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_list_properties(pkg, ray_set_scene, name, variant):
    mode, arith = tc.variant_mode(pkg, variant)
    rays = tc.load_ray_fixture(name)["rays"]
    counts, _ = ac.check_list_properties(tracer(ray_set_scene(name, arith)), rays, mode)
    assert (counts == 0).any() and (counts >= 1).any(), name


def test_every_set_truncates_a_row(pkg, answers):
    """On every set: rays with count == 0 and rays with count > K for each tested K <= 8.  The two
    smallest scenes cannot meet every K: tri1 is one triangle, and no ray of quad_tiny meets more than
    two of quad's three -- the floor there is what the model gives (its largest hit set, asserted)."""
    largest = {"tri1_tiny": 1, "quad_tiny": 2}
    for name in tc.RAY_SETS:
        counts, _ = answers(name)
        assert (counts == 0).any(), name
        if name in largest:
            assert int(ac.model(name)[0].max()) == largest[name] == int(counts.max()), name
        for K in ac.PREFIX_K:
            if K < largest.get(name, 9):
                assert (counts > K).any(), (name, K, int(counts.max()))


def test_floors_that_keep_the_checks_from_passing_vacuously(pkg, answers):
    """Asserted on the CPU path's output at max_hits = 32, exact_fast."""
    counts, rows = answers(tc.LATTICE)
    assert (counts > 16).sum() >= 10 and (counts > 8).sum() >= 50, ((counts > 16).sum(), (counts > 8).sum())
    tied = ac.rows_with_equal_t(counts, rows)
    assert tied.sum() >= 500, int(tied.sum())                         # tie order is decided by prim
    # ... at least once between a z = 0 triangle and its "-0" twin (other ties may sit between the two)
    per = 2 * tc.LATTICE_CELLS * tc.LATTICE_CELLS
    twin_ties = 0
    for k in np.flatnonzero(tied):
        kept = min(int(counts[k]), ac.MAX_HITS)
        pk, tk = rows["prim"][k, :kept], rows["t"][k, :kept]
        for i in np.flatnonzero(pk < per):
            j = np.flatnonzero(pk == pk[i] + 3 * per)
            twin_ties += int(len(j) and tk[j[0]] == tk[i])
    assert twin_ties >= 1
    # rays where a brute force over all 128 triangles accepts a triangle the walk does not: the definition matters
    brute = ac.brute_force_counts(tc.LATTICE)
    assert (brute >= counts).all()                                    # the walk's set is a subset
    assert (brute > counts).sum() >= 5, int((brute > counts).sum())
    counts, _ = answers("dragon_octants")
    assert (counts > 4).sum() >= 100 and (counts > 8).sum() >= 10, ((counts > 4).sum(), (counts > 8).sum())
    counts, _ = answers("dragon_adversarial")
    assert (counts > 4).sum() >= 20, int((counts > 4).sum())


def test_threads_do_not_change_the_answer(pkg, ray_set_scene):
    rays = tc.load_ray_fixture("dragon_octants")["rays"]
    sc = ray_set_scene("dragon_octants", 0)
    c1, r1, s1 = sc.trace_all(rays, max_hits=8, threads=1)
    c8, r8, s8 = sc.trace_all(rays, max_hits=8, threads=8)
    assert np.array_equal(c1, c8) and ac.rows_equal(r1, r8)
    assert (s1["node_pairs"], s1["tri_tests"], s1["hits"]) == (s8["node_pairs"], s8["tri_tests"], s8["hits"])


def test_refusals(pkg, ray_set_scene):
    """Each argument rule returns its status, and the scene answers a closest query identically afterwards."""
    sc = ray_set_scene("dragon_adversarial", 0)
    rays = np.ascontiguousarray(tc.load_ray_fixture("dragon_adversarial")["rays"][:64])
    before = sc.trace(rays, closest=True, occluded=True)
    L = pkg.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    cnt = np.zeros(64, np.uint32)
    rows = np.zeros((64, 33), pkg.HIT_DTYPE)
    call = lambda n, mode, K, c, h: L.ceres_trace_rays_all_cpu(sc._h, vp(rays), n, mode, K, c, h, None, 0)   # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -6
    assert call(64, 0, 0, vp(cnt), vp(rows)) == EINVAL                # a hit buffer with max_hits = 0
    assert call(64, 0, 33, vp(cnt), vp(rows)) == EINVAL               # max_hits > CERES_MAX_HITS
    assert call(64, 0, 8, None, None) == EINVAL                       # neither output
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY, 0x80):
        assert call(64, bad, 8, vp(cnt), vp(rows)) == EINVAL, bad
    assert call(1 << 31, 0, 8, vp(cnt), vp(rows)) == EUNSUPPORTED
    assert L.ceres_trace_rays_all_cpu(sc._h, None, 64, 0, 8, vp(cnt), vp(rows), None, 0) == EINVAL   # null rays
    assert not cnt.any() and not rows.view(np.uint32).any()           # nothing was written
    assert call(64, 0, 77, vp(cnt), None) == 0                        # count-only: max_hits ignored
    assert np.array_equal(cnt, sc.trace_all(rays, max_hits=1)[0])
    with pytest.raises(pkg.CeresError):
        sc.trace_all(rays, max_hits=0)
    with pytest.raises(pkg.CeresError):
        sc.trace_all(rays, max_hits=33)
    with pytest.raises(pkg.CeresError):
        sc.trace_all(rays, mode=pkg.MODE_PRIMARY)
    with pytest.raises(pkg.CeresError):
        sc.trace_all(np.zeros((3, 7), np.float32))
    st = pkg._Stats(rays=7, hits=7, node_pairs=7, tri_tests=7)
    assert L.ceres_trace_rays_all_cpu(sc._h, None, 0, 0, 8, vp(cnt), vp(rows), ctypes.byref(st), 0) == 0   # n_rays = 0
    assert (st.rays, st.hits, st.node_pairs, st.tri_tests) == (0, 0, 0, 0)
    c0, r0, s0 = sc.trace_all(np.zeros((0, 8), np.float32), max_hits=4)
    assert c0.shape == (0,) and r0.shape == (0, 4) and s0["rays"] == 0
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"], f64=True)
    d = pkg.CpuScene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_all_cpu(d._h, vp(rays), 64, 0, 8, vp(cnt), vp(rows), None, 0) == EUNSUPPORTED
    finally:
        d.close()
    assert pkg.MAX_HITS == ac.MAX_HITS == 32
    assert "ceres_trace_all_k" in L.ceres_kernel_names().decode().split(",")
    after = sc.trace(rays, closest=True, occluded=True)
    assert tc.hits_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_cli_cpu_all_hits(pkg, ray_set_scene, tmp_path):
    """./render --cpu --rays --all-hits K on tests/golden/lattice.obj: the files hold CpuScene.trace_all's
    bytes; K = 0 with --counts-out alone is the count-only query; --double: the library's refusal,
    status 1; bad combinations are bad usage (status 2)."""
    rays = tc.load_ray_fixture(tc.LATTICE)["rays"]
    cfg = tc.ray_set_config(tc.LATTICE)
    counts, rows, st = ray_set_scene(tc.LATTICE, 0).trace_all(rays, max_hits=5)
    rf, hf, cf = tmp_path / "rays.bin", tmp_path / "hits.bin", tmp_path / "counts.bin"
    rf.write_bytes(rays.tobytes())
    base = [pkg.CLI_PATH, tc.LATTICE_OBJ]
    if cfg.get("rotate"):
        base += ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    base += ["--exact", "--cpu", "--rays", str(rf)]
    run = lambda *a: subprocess.run(base + list(a), capture_output=True, text=True, timeout=120)   # noqa: E731
    r = run("--json", "--all-hits", "5", "--hits-out", str(hf), "--counts-out", str(cf))
    assert r.returncode == 0, r.stderr
    assert hf.read_bytes() == rows.tobytes() and cf.read_bytes() == counts.tobytes()
    assert '"rays": %d, "hits": %d, "max_hits": 5' % (len(rays), st["hits"]) in r.stdout
    os.remove(cf)
    r = run("--all-hits", "0", "--counts-out", str(cf))
    assert r.returncode == 0 and cf.read_bytes() == counts.tobytes()
    r = run("--all-hits", "5", "--hits-out", str(hf), "--double")
    assert r.returncode == 1 and "float scenes" in r.stderr
    r = run("--all-hits", "33", "--hits-out", str(hf))
    assert r.returncode == 1 and "max_hits" in r.stderr
    for bad in (("--all-hits", "5"), ("--all-hits", "0", "--hits-out", str(hf)), ("--counts-out", str(cf), "--hits-out", str(hf)),
                ("--all-hits", "5", "--hits-out", str(hf), "--occluded-out", str(cf)), ("--all-hits", "-1", "--hits-out", str(hf))):
        assert run(*bad).returncode == 2, bad
