"""Ray queries on double-precision scenes, CPU path (ceres_trace_rays_cpu_f64, CpuScene.trace on a double
scene, `./render --cpu --double --rays`): closest hit and occlusion for caller-supplied ray64 records.

The double queries are pinned by the reference's own render<double> records through rays rebuilt on
the host (the contraction-free build: camera_rays64 / shadow_rays64; the CMake build: an exact fma),
with its Statistics, by a brute force over all triangles that knows no BVH, and by what the
reference's traverser returned for the stored caller rays of tests/golden/rays64/ (windows, non-finite
rays, the lattice's exact ties) in its two double builds.  No tolerance anywhere.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import trace64_common as t64


@pytest.fixture(scope="module")
def cpu_scene(pkg):
    cache = {}

    def get(name, build="exact"):
        if (name, build) not in cache:
            if name in t64.BRUTE_SCENES and name != "quad":
                mesh, bvh = t64.brute_scene(name)
            else:
                _, mesh, bvh, _, _, _, _ = t64.fixture(name, build)
            cache[name, build] = pkg.CpuScene(mesh, bvh)
        return cache[name, build]

    yield get
    for s in cache.values():
        s.close()


def tracer(scene, **kw):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded, **kw)


@pytest.mark.parametrize("name", t64.EXACT_FIXTURES)
def test_closest_hit_equals_reference_double_records(pkg, cpu_scene, name):
    t64.check_closest_against_fixture(pkg, tracer(cpu_scene(name)), name)


@pytest.mark.parametrize("name", t64.OCCLUSION_FIXTURES)
def test_occlusion_equals_reference_shadow_flags(pkg, cpu_scene, name):
    t64.check_occlusion_against_fixture(pkg, tracer(cpu_scene(name)), name)


@pytest.mark.parametrize("name", t64.REF_FIXTURES)
def test_closest_hit_equals_reference_cmake_build_records(pkg, cpu_scene, name):
    """CERES_MODE_FMA on an ARITH_FMA scene, rays rebuilt with a correctly rounded fma."""
    t64.check_closest_against_fixture(pkg, tracer(cpu_scene(name, "ref")), name, build="ref")


@pytest.mark.parametrize("which", t64.BRUTE_SCENES)
def test_closest_hit_equals_brute_force(pkg, cpu_scene, which):
    """The set's conditions (ties within 1 %, hits, misses, a hit its own window rejects) are asserted
    from numpy alone before the code under test runs."""
    t64.check_against_brute_force(pkg, tracer(cpu_scene(which)), which)


def test_occlusion_is_closest_found_a_hit_on_adversarial_rays(pkg, cpu_scene):
    rays = t64.adversarial_rays()
    for mode, build in t64.modes(pkg):
        hits, occ, st = cpu_scene(t64.DRAGON, build).trace(rays, mode=mode, closest=True, occluded=True)
        assert np.array_equal(occ, (hits["prim"] >= 0).astype(np.uint8)), mode
        t64.assert_misses_are_zero(hits)
        t64.check_adversarial_input(rays, hits)
        assert st["rays"] == len(rays) and st["hits"] == int(occ.sum())


@pytest.mark.parametrize("name", t64.TINY_FIXTURES)
def test_tiny_tree_rays_meet_their_conditions(pkg, cpu_scene, name):
    rays = t64.tiny_tree_rays(name)
    open_rays = np.array(rays)
    open_rays[:, 6:8] = (0, t64.DBL_MAX)
    for mode, build in t64.modes(pkg):
        sc = cpu_scene(name, build)
        hits, occ, _ = sc.trace(rays, mode=mode, closest=True, occluded=True)
        t64.check_tiny_tree_input(name, hits, sc.trace(open_rays, mode=mode, closest=True)[0])
        assert np.array_equal(occ, (hits["prim"] >= 0).astype(np.uint8)), mode


def test_nan_window_is_the_empty_window(pkg, cpu_scene):
    """A NaN tmin or tmax: a miss after one traversal step (render_cpu.cpp's float rule), also on rays
    that would hit; on tri1, whose root is a leaf, one triangle test and no step."""
    for name, steps in (("quad", 1), ("tri1", 0)):
        cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(name)
        rays = pkg.camera_rays64(basis, cfg["W"], cfg["H"])[rec["pixel"][rec["prim"] >= 0]][:3].copy()
        sc = cpu_scene(name)
        assert (sc.trace(rays, closest=True)[0]["prim"] >= 0).all()
        rays[0, 6], rays[1, 7], rays[2, 6:8] = np.nan, np.nan, np.nan
        for k in range(3):
            hits, occ, st = sc.trace(rays[k:k + 1], closest=True, occluded=True)
            assert hits["prim"][0] == -1 and occ[0] == 0
            assert st["node_pairs"] == steps and st["tri_tests"] == (0 if steps else len(mesh)), (name, k)


def test_interface_details(pkg, cpu_scene):
    sc = cpu_scene(t64.DRAGON)
    rays = t64.adversarial_rays()
    h1, o1, _ = sc.trace(rays, closest=True, occluded=True, threads=1)
    h8, o8, _ = sc.trace(rays, closest=True, occluded=True, threads=8)
    assert t64.hits_equal(h1, h8) and np.array_equal(o1, o8)
    only_h, none_o, _ = sc.trace(rays, closest=True, occluded=False)
    none_h, only_o, _ = sc.trace(rays, closest=False, occluded=True)
    assert none_o is None and none_h is None and t64.hits_equal(only_h, h1) and np.array_equal(only_o, o1)
    h0, o0, st = sc.trace(np.zeros((0, 8), np.float64), closest=True, occluded=True)      # n_rays = 0: a no-op
    assert len(h0) == 0 and len(o0) == 0 and st["rays"] == 0
    L = pkg.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    r = np.ascontiguousarray(rays[:4])
    h = np.zeros(4, pkg.HIT64_DTYPE)
    assert L.ceres_trace_rays_cpu_f64(sc._h, None, 0, 0, vp(h), None, None, 0) == 0
    assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 4, 0, vp(h), None, None, 0) == 0
    assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 4, pkg.MODE_FMA, vp(h), None, None, 0) == 0
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY, 0x80):
        assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 4, bad, vp(h), None, None, 0) == -1, bad   # CERES_EINVAL
        with pytest.raises(pkg.CeresError, match="error -1"):
            sc.trace(r, mode=bad)
    for robust in (pkg.MODE_ROBUST, pkg.MODE_ROBUST | pkg.MODE_FMA):                               # float-only
        assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 4, robust, vp(h), None, None, 0) == -6     # CERES_EUNSUPPORTED
    assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 4, 0, None, None, None, 0) == -1               # both outputs NULL
    with pytest.raises(pkg.CeresError, match="error -1"):
        sc.trace(r, closest=False, occluded=False)
    assert L.ceres_trace_rays_cpu_f64(sc._h, vp(r), 1 << 31, 0, vp(h), None, None, 0) == -6
    with pytest.raises(pkg.CeresError):
        sc.trace(np.zeros((3, 7), np.float64))
    # precision mismatches, both ways
    assert L.ceres_trace_rays_cpu(sc._h, vp(r), 4, 0, vp(h), None, None, 0) == -6                  # float call, double scene
    mesh, bvh, _ = pkg.prepare(pkg.configs.CONFIGS["tri1"])
    f = pkg.CpuScene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_cpu_f64(f._h, vp(r), 4, 0, vp(h), None, None, 0) == -6           # double call, float scene
    finally:
        f.close()
    for sym in ("ceres_trace_rays_f64", "ceres_trace_rays_f64_device", "ceres_trace_rays_cpu_f64"):
        assert sym in pkg.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "ceres_trace_rays64_k" in L.ceres_kernel_names().decode().split(",")
    assert pkg.HIT64_DTYPE.itemsize == 32 and pkg.HIT64_DTYPE.names == ("prim", "pad", "t", "u", "v")


def test_cli_cpu_double_rays(pkg, cpu_scene, tmp_path):
    """./render --cpu --double --rays on tests/golden/tri1.obj with the fixture's camera rays: the files
    hold the API's bytes; a file that is not a whole number of 64-byte records is bad usage (status 2)."""
    name = "tri1"
    cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(name)
    rays = pkg.camera_rays64(basis, cfg["W"], cfg["H"])
    hits, occ, st = cpu_scene(name).trace(rays, closest=True, occluded=True)
    assert st["hits"] > 0
    rf, hf, of = tmp_path / "rays.bin", tmp_path / "hits.bin", tmp_path / "occ.bin"
    rf.write_bytes(rays.tobytes())
    args = [os.path.join(os.path.dirname(__file__), "golden", "tri1.obj")]
    if cfg["rotate"]:
        args += ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    r = subprocess.run([pkg.CLI_PATH] + args + ["--exact", "--cpu", "--double", "--json", "--rays", str(rf), "--hits-out", str(hf),
                                                "--occluded-out", str(of)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert hf.read_bytes() == hits.tobytes() and of.read_bytes() == occ.tobytes()
    assert '"rays": %d, "hits": %d' % (len(rays), st["hits"]) in r.stdout and '"ms"' in r.stdout
    (tmp_path / "short.bin").write_bytes(rays.tobytes()[:-32])        # whole 32-byte records, not 64-byte ones
    r = subprocess.run([pkg.CLI_PATH] + args + ["--exact", "--cpu", "--double", "--rays", str(tmp_path / "short.bin"),
                                                "--hits-out", str(hf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "64" in r.stderr


# ---------------------------------------------------------------- rays the reference traced itself

@pytest.fixture(scope="module")
def ray_set_scene(pkg):
    """get(set, build) -> the CpuScene of a double ray set's scene (tests/golden/rays64/<set>.npz)."""
    cache = {}

    def get(name, build="exact"):
        key = (t64.ray_set_config(name)["obj"], build)
        if key not in cache:
            cache[key] = pkg.CpuScene(*t64.ray_set_scene(name, build))
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_ray_set_generators_reproduce_the_stored_rays(name):
    assert t64.ray_set_rays(name).tobytes() == t64.load_ray_fixture64(name)["rays"].tobytes()


def test_lattice64_set_meets_its_floors():
    """The float set's floors on the double builds' stored answers (no robust variants here)."""
    import trace_common as tc
    fx = t64.load_ray_fixture64(t64.LATTICE64)
    assert np.array_equal(fx["rays"], tc.load_ray_fixture(tc.LATTICE)["rays"].astype(np.float64))
    tc.check_lattice_conditions(fx, robust=False)


def test_adversarial64_set_holds_its_special_rays():
    """Stored whole: the 21 specials at the end (axis rays, the zero direction, NaN / +-inf components,
    tmin > tmax), hits and misses among the others."""
    fx = t64.load_ray_fixture64("dragon_adversarial64")
    rays, ref = fx["rays"], fx["exact_fast"]
    assert len(rays) == 4099
    t64.check_adversarial_input(rays, {"prim": ref["prim"]})
    assert np.isnan(rays[-21:]).any(axis=1).sum() == 2 and (rays[-2:, 6] > rays[-2:, 7]).all()


@pytest.mark.parametrize("variant", t64.RAY_VARIANTS64)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_caller_rays_equal_the_reference_traverser(pkg, ray_set_scene, name, variant):
    """Every stored double ray, the non-finite ones included: prim, t, u, v, occluded of the reference's
    traverse(ray, intersector) in its double builds, and its Statistics summed over the rays without
    a NaN and over the rays with one."""
    sc = ray_set_scene(name, t64.variant_mode(pkg, variant)[1])
    t64.check_against_ray_fixture64(pkg, tracer(sc), name, variant, stats=True)
    t64.check_against_ray_fixture64(pkg, tracer(sc), name, variant, stats=False)
