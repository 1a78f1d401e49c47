"""Ray queries on the CPU path (ceres_trace_rays_cpu, CpuScene.trace, `./render --cpu --rays`): closest
hit and occlusion for caller-supplied rays, the reference's traverser.traverse(ray, intersector)
(single_ray_traverser.hpp:68-126) for any bvh::Ray{origin, direction, tmin, tmax}.

The pin is the reference itself: tests/golden/<name>.records.npz holds the contraction-free
reference build's per-pixel {prim, t, u, v, shadow}, and the rays behind them are rebuilt on the host
bit for bit (camera_rays / shadow_rays).  Every recorded pixel and every shadow ray of the named
fixtures is compared, with no tolerance.  For rays a camera never makes (windows, unnormalised
directions, signed zeros, non-finite components) tests/golden/rays/<set>.npz holds what the
reference's traverser returned in its four builds, ray by ray.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import trace_common as tc


@pytest.fixture(scope="module")
def cpu_scene(pkg):
    cache = {}

    def get(name, arith=0):
        if (name, arith) not in cache:
            _, mesh, bvh, _, _, _, _ = tc.fixture(name, arith)
            cache[name, arith] = pkg.CpuScene(mesh, bvh)
        return cache[name, arith]

    yield get
    for s in cache.values():
        s.close()


def tracer(scene, **kw):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded, **kw)


@pytest.mark.parametrize("name", tc.CLOSEST_FIXTURES)
def test_closest_hit_equals_reference_records(pkg, cpu_scene, name):
    tc.check_closest_against_fixture(pkg, tracer(cpu_scene(name)), name)


@pytest.mark.parametrize("name", tc.OCCLUSION_FIXTURES)
def test_occlusion_equals_reference_shadow_flags(pkg, cpu_scene, name):
    tc.check_occlusion_against_fixture(pkg, tracer(cpu_scene(name)), name)


def test_direction_scale(pkg, cpu_scene):
    tc.check_scale(pkg, tracer(cpu_scene(tc.DRAGON)))


def test_window(pkg, cpu_scene):
    tc.check_window(pkg, tracer(cpu_scene(tc.DRAGON)))


def test_occlusion_is_closest_found_a_hit(pkg, cpu_scene):
    """On the adversarial set, in {exact, FMA} x {fast, robust}."""
    rays = tc.adversarial_rays()
    seen = 0
    for mode, arith in tc.modes(pkg):
        hits, occ, st = cpu_scene(tc.DRAGON, arith).trace(rays, mode=mode, closest=True, occluded=True)
        assert np.array_equal(occ, (hits["prim"] >= 0).astype(np.uint8)), mode
        miss = hits["prim"] < 0
        assert not hits["t"][miss].view(np.uint32).any()
        assert st["rays"] == len(rays) and st["hits"] == int(occ.sum())
        seen += int(occ.sum())
    assert seen > 400                                                # the set does hit the mesh


@pytest.mark.parametrize("name", tc.TINY_FIXTURES)
def test_tiny_tree_rays_meet_their_conditions(pkg, cpu_scene, name):
    """The ray set of the GPU smallest-trees comparison: hits, misses, hits its own window rejects, and
    misses with tmin <= -1 that fail a u / v / w stage; occlusion == the closest query finds a hit."""
    rays = tc.tiny_tree_rays(name)
    open_rays = np.array(rays)
    open_rays[:, 6:8] = (0, tc.FLT_MAX)
    for mode, arith in tc.modes(pkg):
        sc = cpu_scene(name, arith)
        hits, occ, _ = sc.trace(rays, mode=mode, closest=True, occluded=True)
        tc.check_tiny_tree_input(name, rays, hits, sc.trace(open_rays, mode=mode, closest=True)[0])
        assert np.array_equal(occ, (hits["prim"] >= 0).astype(np.uint8)), mode


def test_interface_details(pkg, cpu_scene):
    sc = cpu_scene(tc.DRAGON)
    rays = tc.adversarial_rays()
    h1, o1, _ = sc.trace(rays, closest=True, occluded=True, threads=1)
    h8, o8, _ = sc.trace(rays, closest=True, occluded=True, threads=8)
    assert tc.hits_equal(h1, h8) and np.array_equal(o1, o8)
    only_h, none_o, _ = sc.trace(rays, closest=True, occluded=False)
    none_h, only_o, _ = sc.trace(rays, closest=False, occluded=True)
    assert none_o is None and none_h is None and tc.hits_equal(only_h, h1) and np.array_equal(only_o, o1)
    h0, o0, st = sc.trace(np.zeros((0, 8), np.float32), closest=True, occluded=True)      # n_rays = 0: a no-op
    assert len(h0) == 0 and len(o0) == 0 and st["rays"] == 0
    L = pkg.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731
    r = np.ascontiguousarray(rays[:4])
    h = np.zeros(4, pkg.HIT_DTYPE)
    assert L.ceres_trace_rays_cpu(sc._h, None, 0, 0, vp(h), None, None, 0) == 0
    for bad in (pkg.MODE_PRIMARY, pkg.MODE_QBVH4, pkg.MODE_FMA | pkg.MODE_PRIMARY, 0x80):
        assert L.ceres_trace_rays_cpu(sc._h, vp(r), 4, bad, vp(h), None, None, 0) == -1, bad       # CERES_EINVAL
        with pytest.raises(pkg.CeresError):
            sc.trace(r, mode=bad)
    assert L.ceres_trace_rays_cpu(sc._h, vp(r), 4, 0, None, None, None, 0) == -1                   # both outputs NULL
    with pytest.raises(pkg.CeresError):
        sc.trace(r, closest=False, occluded=False)
    assert L.ceres_trace_rays_cpu(sc._h, vp(r), 1 << 31, 0, vp(h), None, None, 0) == -6            # CERES_EUNSUPPORTED
    with pytest.raises(pkg.CeresError):
        sc.trace(np.zeros((3, 7), np.float32))
    cfg = pkg.configs.CONFIGS["tri1"]
    mesh, bvh, _ = pkg.prepare(cfg, f64=True)
    d = pkg.CpuScene(mesh, bvh)
    try:
        assert L.ceres_trace_rays_cpu(d._h, vp(r), 4, 0, vp(h), None, None, 0) == -6               # a double scene
    finally:
        d.close()


def test_cli_cpu_rays(pkg, cpu_scene, tmp_path):
    """./render --cpu --rays on tests/golden/tri1.obj with the fixture's camera rays: the files hold
    the API's bytes; a truncated ray file is bad usage (status 2)."""
    name = "tri1"
    cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(name)
    rays = pkg.camera_rays(basis, cfg["W"], cfg["H"])
    hits, occ, st = cpu_scene(name).trace(rays, closest=True, occluded=True)
    rf, hf, of = tmp_path / "rays.bin", tmp_path / "hits.bin", tmp_path / "occ.bin"
    rf.write_bytes(rays.tobytes())
    args = [os.path.join(os.path.dirname(__file__), "golden", "tri1.obj")]
    if cfg["rotate"]:
        args += ["--rotate", cfg["rotate"][0], repr(cfg["rotate"][1])]
    r = subprocess.run([pkg.CLI_PATH] + args + ["--exact", "--cpu", "--json", "--rays", str(rf), "--hits-out", str(hf),
                                                "--occluded-out", str(of)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert hf.read_bytes() == hits.tobytes() and of.read_bytes() == occ.tobytes()
    assert '"rays": %d, "hits": %d' % (len(rays), st["hits"]) in r.stdout and '"ms"' in r.stdout
    (tmp_path / "short.bin").write_bytes(rays.tobytes()[:-5])
    r = subprocess.run([pkg.CLI_PATH] + args + ["--exact", "--cpu", "--rays", str(tmp_path / "short.bin"), "--hits-out", str(hf)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "32" in r.stderr


# ---------------------------------------------------------------- rays the reference traced itself

@pytest.fixture(scope="module")
def ray_set_scene(pkg):
    """get(set, arith) -> the CpuScene of a ray set's scene (tests/golden/rays/<set>.npz)."""
    cache = {}

    def get(name, arith=0):
        key = ("proc300" if name == "proc300_window" else tc.ray_set_config(name)["obj"], arith)
        if key not in cache:
            cache[key] = pkg.CpuScene(*tc.ray_set_scene(name, arith))
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_ray_set_generators_reproduce_the_stored_rays(name):
    """The fixtures and the GPU-against-CPU tests speak of the same input, byte for byte."""
    assert tc.ray_set_rays(name).tobytes() == tc.load_ray_fixture(name)["rays"].tobytes()


def test_octant_set_layout():
    """Stored order: 24 wavefronts uniform in their octant (each octant thrice), one uniform but for
    a lane, and a uniform tail of 37."""
    octant = tc.ray_octant(tc.load_ray_fixture("dragon_octants")["rays"])
    assert len(octant) == tc.OCT_N == 64 * 25 + 37
    waves = [set(octant[k:k + 64].tolist()) for k in range(0, len(octant), 64)]
    assert waves[:24] == [{g // 3} for g in range(24)]
    assert waves[24] == {tc.OCT_MIXED[0], tc.OCT_MIXED[1]} and (octant[64 * 24:64 * 25] != tc.OCT_MIXED[0]).sum() == 1
    assert waves[25] == {tc.OCT_TAIL[0]}


def test_ray_fixtures_are_not_vacuous(pkg, ray_set_scene):
    tc.check_ray_fixture_conditions(pkg, ray_set_scene)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_caller_rays_equal_the_reference_traverser(pkg, ray_set_scene, name, variant):
    """Every stored ray, the non-finite ones included: prim, t, u, v, occluded of the reference's
    traverse(ray, intersector), and its Statistics summed over the rays without a NaN and over the
    rays with one."""
    sc = ray_set_scene(name, tc.variant_mode(pkg, variant)[1])
    tc.check_against_ray_fixture(pkg, tracer(sc), name, variant, stats=True)
    tc.check_against_ray_fixture(pkg, tracer(sc), name, variant, stats=False)


def test_lattice_obj_is_the_generators():
    """tests/golden/lattice.obj byte for byte lattice_obj_text(): the integers and "-0" as coordinate
    strings, 128 triangles."""
    with open(tc.LATTICE_OBJ, "rb") as f:
        text = f.read()
    assert text == tc.lattice_obj_text().encode()
    coords = {w for line in text.decode().splitlines() if line.startswith("v ") for w in line.split()[1:]}
    assert coords == {"-0", "0", "1", "2", "3", "4"}
    _, mesh, _ = tc.lattice(0)
    assert len(mesh) == 128 == sum(line.startswith(b"f ") for line in text.splitlines())
    twins = tc.lattice_twins()
    a, b = mesh.tri[twins[:32]], mesh.tri[twins[32:]]
    assert np.array_equal(a, b) and (np.signbit(b[:, 2]) & ~np.signbit(a[:, 2])).all()    # coincident, p0.z = -0 against +0


def test_lattice_set_meets_its_floors():
    """On the reference's stored answers alone: at least 50 hits each with u, v, w == 0, 20 each with
    t == tmin, t == tmax and a negative-zero u or v, 50 on a triangle with a coincident twin; fast and
    robust differ on at least 100 rays; the contracted builds equal the contraction-free ones on
    every ray (the set is exact); no uniform wavefront in stored order, at least four per octant
    in octant order."""
    tc.check_lattice_conditions(tc.load_ray_fixture(tc.LATTICE))
