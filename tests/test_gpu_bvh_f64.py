"""GPU build of the double-precision BVH (csrc/bvh_build64.hip): the gfx950 builder must produce the
reference's Bvh<double> -- BinnedSahBuilder<Bvh<double>,16> -- bit for bit in both arithmetics: the same
topology, node boxes (sign of zero included) and primitive_indices, compared through the
numbering-independent canonical sha256 of tests/golden/make_golden_f64.py against (a) the hashes the
reference's own two double builds produced (tests/golden/f64) and (b) the host double builder
(ceres_bvh_build_f64_arith, pinned to the reference by tests/test_host_scene_f64.py) on adversarial soups:
sizes around the small-subtree threshold (256) and the binning chunk (4096), signed zeros and equal
coordinates (the reduction's tie-break), a flat axis, duplicates, clusters, coordinates that only a double
tells apart (`fine`), coordinates no float holds (`wide`), and the non-finite soups of tests/soup_common.py
widened to double."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN

import configs
import soup_common as sc

gpu_test = pytest.mark.gpu

F64 = os.path.join(GOLDEN, "f64")
NAMES = sorted(f[:-5] for f in os.listdir(F64) if f.endswith(".json"))
# one config per distinct mesh (+ rotation)
_MESHES = {}
for _n in NAMES:
    _c = configs.CONFIGS[_n]
    _MESHES.setdefault((_c["obj"], _c["proc"], _c["rotate"]), _n)
MESH_CONFIGS = sorted(_MESHES.values())

EINVAL, EUNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


def canon(bvh):
    import make_golden_f64
    assert bvh.nodes.dtype == np.uint64
    return make_golden_f64.canonical_bvh64_sha(bvh.nodes.tobytes(), bvh.prim.tobytes())


def _mesh(pkg, cfg, arith=0):
    mesh = pkg.proc_mesh_f64(cfg["proc"], arith) if cfg.get("proc") else pkg.load_obj_f64(configs.obj_path(cfg), arith)
    if cfg.get("rotate"):
        pkg.rotate_triangles(mesh, cfg["rotate"][0], cfg["rotate"][1], arith)
    return mesh


@gpu_test
@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("name", MESH_CONFIGS)
def test_gpu_bvh64_matches_reference_fixture(gpu, name, arith):
    """Both reference double builds: the contraction-free one and the CMake-flag one, whose SAH costs
    contract into FMA (oracle/contraction_sites.txt)."""
    pkg = gpu
    meta = json.load(open(os.path.join(F64, name + ".json")))
    mesh = _mesh(pkg, configs.CONFIGS[name], arith)
    assert mesh.f64
    bvh = pkg.build_bvh_gpu(mesh, arith=arith)
    want = meta["ref_scene"]["bvh_canonical_sha256"] if arith else meta["bvh_canonical_sha256"]
    assert canon(bvh) == want
    if not arith:
        assert bvh.nodes.shape[0] == meta["n_nodes"]
    assert np.array_equal(np.sort(bvh.prim), np.arange(len(mesh), dtype=np.uint64))


def soup64(rng, n, kind):
    """Adversarial triangle soups as bvh::Triangle<double> rows {p0, e1 = p0 - p1, e2 = p2 - p0, n}: the kinds
    of tests/test_gpu_bvh.py in float64, and two that a float intermediate anywhere would break."""
    if kind in ("uniform", "wide"):
        p = rng.random((n, 3, 3)) * 10 - 5
        if kind == "wide":                          # infinite as floats; the SAH areas (~2^806) stay finite in double
            p = p * 2.0 ** 400
    elif kind == "grid":                            # many equal coordinates, exact zeros of both signs
        p = rng.integers(-3, 4, size=(n, 3, 3)).astype(np.float64)
        p[rng.random((n, 3, 3)) < 0.3] = -0.0
    elif kind == "flat":                            # every triangle in z = 0 (flat axis: 1/0 bin scale)
        p = rng.random((n, 3, 3))
        p[..., 2] = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0)
    elif kind == "dups":                            # few distinct triangles, repeated (one-sided partitions)
        base = rng.random((7, 3, 3))
        p = base[rng.integers(0, 7, size=n)]
    elif kind == "clustered":                       # tight clusters far apart (deep, unbalanced splits)
        c = rng.random((5, 3)) * 1e4
        p = c[rng.integers(0, 5, size=n)][:, None, :] + rng.random((n, 3, 3)) * 1e-3
    elif kind == "fine":                            # 1 + k 2^-40, k < 2^15: distinct doubles, all 1.0f as floats
        p = 1.0 + rng.integers(0, 2 ** 15, size=(n, 3, 3)).astype(np.float64) * 2.0 ** -40
        assert np.all(p.astype(np.float32) == np.float32(1.0)) and (n < 2 or np.unique(p).size > 1)
    else:
        raise ValueError(kind)
    p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
    e1 = p0 - p1
    e2 = p2 - p0
    with np.errstate(over="ignore"):
        nrm = np.cross(e1, e2)
    return np.concatenate([p0, e1, e2, nrm], axis=1).astype(np.float64)


# the smallest sizes at which each mechanism can still go wrong: a root leaf, one split, the 16-triangle leaf
# rule, both sides of the small-subtree threshold -- 64 in a mesh below 65536 triangles, else the float
# builder's 256: 64 / 65, 128 / 129 (two subtrees at the threshold), 65535 / 65536 (the switch itself; from
# there on 256-primitive subtrees hang under large items) -- the float builder's 256 / 257 / 512 / 513, both sides of the kChunk = 4096 workgroup boundary, several large levels
# (the binning workgroup's chunk grows with the mesh, 256 positions up to 32768 + 127 triangles: 32896 is the
# first size with two 64-record runs per wavefront, 70000 has three)
SOUPS = ([("uniform", n) for n in (1, 2, 17, 64, 65, 128, 129, 256, 257, 512, 513, 1500, 4096, 4097, 20000, 32895, 32896,
                                       65535, 65536, 70000)] +
         [("grid", 600), ("grid", 20000), ("flat", 3000), ("dups", 300), ("dups", 5000), ("clustered", 20000),
          ("fine", 300), ("fine", 5000), ("wide", 257), ("wide", 5000)])


def assert_same_tree(pkg, mesh, what=""):
    for arith in (0, 1):
        host = pkg.build_bvh(mesh, arith=arith)
        dev = pkg.build_bvh_gpu(mesh, arith=arith)
        assert dev.nodes.dtype == np.uint64 and host.nodes.dtype == np.uint64
        assert dev.nodes.shape == host.nodes.shape, (what, arith)
        assert np.array_equal(dev.prim, host.prim), (what, arith)  # primitive_indices: same permutation, same order
        assert canon(dev) == canon(host), (what, arith)


@gpu_test
@pytest.mark.parametrize("kind,n", SOUPS, ids=["%s-%d" % c for c in SOUPS])
def test_gpu_bvh64_matches_host_builder(gpu, kind, n):
    pkg = gpu
    tri = soup64(np.random.default_rng(1234 + n), n, kind)
    assert_same_tree(pkg, pkg.Mesh(tri, np.zeros((n, 9), np.float64)), (kind, n))


def _rows(nodes):
    """Numbering-independent: the sorted (bounds, count) rows of a tree."""
    r = np.ascontiguousarray(nodes[:, :7])
    return np.sort(r.view([("", np.uint64)] * 7).ravel())


@gpu_test
def test_gpu_bvh64_full_chunks(gpu):
    """600,000 triangles: the binning workgroups take their full 4096 positions (16 runs per wavefront, from
    491,648 triangles on).  Too many nodes for the canonical walk in a few seconds, so the comparison is the
    primitive order, the node count and the sorted set of (box, count) rows."""
    pkg = gpu
    n = 600000
    tri = soup64(np.random.default_rng(1234 + n), n, "uniform")
    mesh = pkg.Mesh(tri, np.zeros((n, 9), np.float64))
    host, dev = pkg.build_bvh(mesh), pkg.build_bvh_gpu(mesh)
    assert dev.nodes.shape == host.nodes.shape
    assert np.array_equal(dev.prim, host.prim)
    assert np.array_equal(_rows(dev.nodes), _rows(host.nodes))


# ---- non-finite input: the soups of tests/soup_common.py widened to double.  Every case is kept: the host
# double builder returns on each of them (checked on the CPU by the test below, so the list cannot drift).
NONFINITE = list(sc.CASES)


def _soup_mesh(pkg, kind, n):
    tri, _ = sc.soup(kind, n)
    with np.errstate(invalid="ignore"):             # (a signalling NaN widens to its quiet double)
        tri = tri.astype(np.float64)
    return pkg.Mesh(tri, np.zeros((n, 9), np.float64))


@pytest.mark.parametrize("kind,n", NONFINITE, ids=["%s-%d" % c for c in NONFINITE])
def test_host_double_builder_returns_on_the_soups(pkg, kind, n):
    """Not a GPU test: the comparison's other side exists for every listed soup, in both arithmetics."""
    mesh = _soup_mesh(pkg, kind, n)
    assert mesh.f64
    for arith in (0, 1):
        bvh = pkg.build_bvh(mesh, arith=arith)
        assert np.array_equal(np.sort(bvh.prim), np.arange(n, dtype=np.uint64))
        assert 1 <= bvh.nodes.shape[0] <= 2 * n - 1


@gpu_test
@pytest.mark.parametrize("kind,n", NONFINITE, ids=["%s-%d" % c for c in NONFINITE])
def test_gpu_bvh64_matches_host_builder_on_nonfinite_soups(gpu, kind, n):
    """A NaN bound contributes the empty key to the reduction; a NaN centre goes to bin 0; +-inf and the
    default NaN of inf - inf (negative on x86, positive on the GPU) show in no node."""
    assert_same_tree(gpu, _soup_mesh(gpu, kind, n), (kind, n))


# ---- device entry point
def _device_build(pkg, mesh, arith=0):
    import torch
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.zeros((2 * n - 1) * 8, dtype=torch.int64, device="cuda:0")
    d_prim = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device_f64(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream, arith)
    torch.cuda.synchronize()
    nodes = d_nodes[: m * 8].cpu().numpy().view(np.uint64).reshape(-1, 8)
    prim = d_prim.cpu().numpy().view(np.uint32)
    return m, nodes, prim


@gpu_test
def test_device_entry_point_is_deterministic(gpu):
    pkg = gpu
    mesh = _mesh(pkg, configs.CONFIGS["proc_101"])
    host_call = pkg.build_bvh_gpu(mesh)
    m1, nodes1, prim1 = _device_build(pkg, mesh)
    m2, nodes2, prim2 = _device_build(pkg, mesh)
    assert m1 == m2 == host_call.nodes.shape[0]
    assert canon(pkg.Bvh(nodes1, prim1.astype(np.uint64))) == canon(host_call)
    assert nodes1.tobytes() == nodes2.tobytes() and prim1.tobytes() == prim2.tobytes()   # numbering is deterministic
    assert nodes1.tobytes() == host_call.nodes.tobytes()


# ---- refusals
@gpu_test
def test_refusals_launch_nothing(gpu):
    import torch
    pkg = gpu
    L = pkg.lib()
    mesh = _mesh(pkg, configs.CONFIGS["proc_101"])
    n = len(mesh)
    d_tri = torch.from_numpy(np.concatenate([mesh.tri.reshape(-1), np.zeros(2)])).to("cuda:0")
    d_nodes = torch.full(((2 * n - 1) * 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda:0")
    d_prim = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda:0")
    m = ctypes.c_size_t(77)
    t, nd, pr = d_tri.data_ptr(), d_nodes.data_ptr(), d_prim.data_ptr()
    assert t % 16 == 0 and nd % 16 == 0 and pr % 16 == 0
    call = L.ceres_bvh_build_f64_device_arith
    assert call(t, 0, nd, pr, ctypes.byref(m), None, 0) == EINVAL                # empty
    assert call(None, n, nd, pr, ctypes.byref(m), None, 0) == EINVAL             # null pointers
    assert call(t, n, None, pr, ctypes.byref(m), None, 0) == EINVAL
    assert call(t, n, nd, None, ctypes.byref(m), None, 0) == EINVAL
    assert call(t, n, nd, pr, None, None, 0) == EINVAL
    assert call(t, n, nd, pr, ctypes.byref(m), None, 5) == EINVAL                # bad arith
    assert call(t + 8, n, nd, pr, ctypes.byref(m), None, 0) == EINVAL            # triangles off 16-byte alignment
    assert b"aligned" in L.ceres_last_error()
    assert call(t, 2 ** 31, nd, pr, ctypes.byref(m), None, 0) == EUNSUPPORTED
    assert L.ceres_bvh_build_f64_device(t, 0, nd, pr, ctypes.byref(m), None) == EINVAL
    # host-array calls
    nodes, prim, cnt = pkg._u64p(), pkg._u64p(), ctypes.c_size_t()
    tp = pkg._p(mesh.tri, ctypes.c_double)
    g = L.ceres_bvh_build_f64_gpu_arith
    assert g(tp, 0, ctypes.byref(nodes), ctypes.byref(cnt), ctypes.byref(prim), 0, 0) == EINVAL
    assert g(None, n, ctypes.byref(nodes), ctypes.byref(cnt), ctypes.byref(prim), 0, 0) == EINVAL
    assert g(tp, n, ctypes.byref(nodes), ctypes.byref(cnt), ctypes.byref(prim), 0, 5) == EINVAL
    assert g(tp, 2 ** 31, ctypes.byref(nodes), ctypes.byref(cnt), ctypes.byref(prim), 0, 0) == EUNSUPPORTED
    with pytest.raises(pkg.CeresError):
        pkg.build_bvh_device_f64(t, n, nd, pr, arith=5)
    torch.cuda.synchronize()
    assert m.value == 77
    assert bool((d_nodes == 0x5a5a5a5a5a5a5a5a).all()) and bool((d_prim == 0x5a5a5a5a).all())   # nothing was written


# ---- the one asserted timing relation
@gpu_test
def test_gpu_bvh64_dragon_is_faster_than_the_host_build(gpu):
    """The repository's dragon (23,490 triangles) in double: best of 3 after a warm-up, GPU build against the
    host double build on the cores this process may use; both printed.

    Measured on one MI355X with 16 host cores: GPU 1.6 - 1.7 ms, host 2.7 - 5.2 ms over seven runs (the host
    build's time moves with the machine's load).  Before the binning workgroups and the small-subtree threshold
    followed the mesh size the GPU build took 4.4 ms and the relation failed whenever the host was quick
    (DESIGN.md "Double BVH build")."""
    import torch
    pkg = gpu
    mesh = _mesh(pkg, configs.CONFIGS["dragon_333x217"])
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1)).to("cuda:0")
    d_nodes = torch.empty((2 * n - 1) * 8, dtype=torch.int64, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    gpu_ms, host_ms, m = [], [], 0
    for k in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = pkg.build_bvh_device_f64(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream)
        torch.cuda.synchronize()
        if k:
            gpu_ms.append((time.perf_counter() - t0) * 1e3)
    for k in range(4):
        t0 = time.perf_counter()
        pkg.build_bvh(mesh)
        if k:
            host_ms.append((time.perf_counter() - t0) * 1e3)
    print(f"dragon double BVH build: gpu {min(gpu_ms):.1f} ms, host {min(host_ms):.1f} ms ({n} triangles, {m} nodes)")
    assert min(gpu_ms) < min(host_ms)
