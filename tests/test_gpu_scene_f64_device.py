"""Double scenes from device arrays (ceres_scene_create_f64_device, csrc/scene_device64.hip): triangles and
normals in HBM -> GPU double BVH (ceres_bvh_build_f64_device) -> GPU relayout -> every double call, with no
host round trip.  The device relayout numbers its sibling pairs differently from the host one, so the bar is
what the calls return: the scene must be indistinguishable from the one ceres_scene_create_f64 makes from the
host-built BVH of the same mesh -- framebuffer, RGB8, rays / hits, per-pixel records, ray queries, shaded
queries, SAH cost and refit, all bit for bit -- and equal to the reference's own double frame where a fixture
records it.  Malformed trees fail loudly in the validator."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

import configs
import quality_common as qc
import refit_common as rc

pytestmark = pytest.mark.gpu

F64 = os.path.join(GOLDEN, "f64")
SCENES = ["bunny_97x61_primary", "dragon_333x217", "tri1", "quad"]
CASES = [(n, "exact") for n in SCENES] + [("bunny_97x61_primary", "ref"), ("quad", "ref")]


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


def _hex64(hx):
    return np.asarray([int(h, 16) for h in hx], np.uint64).view(np.float64)


def view_of(name, build):
    meta = json.load(open(os.path.join(F64, name + ".json")))
    bb, pose = (meta["ref_basis"], meta["ref_pose"]) if build == "ref" else (meta["basis"], meta["pose"])
    return meta, np.concatenate([_hex64(pose["eye"]), _hex64(bb["dir"] + bb["u"] + bb["v"])]), _hex64(pose["sun"])


class Pair:
    """One mesh as two scenes: host-built BVH + host relayout, and GPU-built BVH + GPU relayout."""

    def __init__(self, pkg, name, arith):
        import torch
        self.pkg = pkg
        self.mesh, self.bvh, _ = pkg.prepare(configs.CONFIGS[name], f64=True, arith=arith)
        n = len(self.mesh)
        self.d_tri = torch.from_numpy(self.mesh.tri.reshape(-1).copy()).to("cuda:0")
        self.d_norm = torch.from_numpy(self.mesh.norm.reshape(-1).copy()).to("cuda:0")
        self.d_nodes = torch.empty(max(2 * n - 1, 1) * 8, dtype=torch.int64, device="cuda:0")
        self.d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        self.m = pkg.build_bvh_device_f64(self.d_tri.data_ptr(), n, self.d_nodes.data_ptr(), self.d_prim.data_ptr(), stream, arith)
        self.dev = pkg.Scene.from_device_f64(self.d_tri.data_ptr(), n, self.d_norm.data_ptr(), self.d_nodes.data_ptr(), self.m,
                                             self.d_prim.data_ptr(), stream=stream)
        self.host = pkg.Scene(self.mesh, self.bvh)

    def close(self):
        self.dev.close()
        self.host.close()


@pytest.fixture(scope="module")
def pairs(gpu):
    made = {}

    def get(name, build="exact"):
        if (name, build) not in made:
            made[name, build] = Pair(gpu, name, 1 if build == "ref" else 0)
        return made[name, build]
    yield get
    for p in made.values():
        p.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name,build", CASES, ids=["%s-%s" % c for c in CASES])
def test_device_scene_equals_host_scene(gpu, pairs, name, build):
    pkg = gpu
    cfg = configs.CONFIGS[name]
    meta, basis, sun = view_of(name, build)
    p = pairs(name, build)
    assert p.dev.f64 and p.m == p.bvh.nodes.shape[0]
    W, H = cfg["W"], cfg["H"]
    mode = pkg.cfg_mode(cfg, 1 if build == "ref" else 0)
    px, rgb, st = p.dev.render(basis, sun, W, H, mode=mode)
    hpx, hrgb, hst = p.host.render(basis, sun, W, H, mode=mode)
    assert px.dtype == np.float64
    assert np.array_equal(bits(px), bits(hpx))
    assert np.array_equal(rgb, hrgb)
    assert (st["rays"], st["hits"]) == (hst["rays"], hst["hits"]) == (meta[build]["rays"], meta[build]["hits"])
    assert hashlib.sha256(pkg.ppm(W, H, rgb)).hexdigest() == meta["ppm_sha256"][build]     # the reference's own frame
    prim, tuv, sh, _ = p.dev.records(basis, sun, W, H, mode=mode)
    hprim, htuv, hsh, _ = p.host.records(basis, sun, W, H, mode=mode)
    assert np.array_equal(prim, hprim) and np.array_equal(sh, hsh)
    hit = hprim >= 0
    assert np.array_equal(bits(tuv)[hit], bits(htuv)[hit])
    qmode = pkg.MODE_FMA if build == "ref" else 0
    rays = pkg.camera_rays64(basis, W, H, 1 if build == "ref" else 0)
    hits, occ, _ = p.dev.trace(rays, mode=qmode, closest=True, occluded=True)
    hhits, hocc, _ = p.host.trace(rays, mode=qmode, closest=True, occluded=True)
    assert hits.tobytes() == hhits.tobytes()
    assert occ.tobytes() == hocc.tobytes()
    assert int((hits["prim"] >= 0).sum()) > 0
    spx, _, shits, sstat, _ = p.dev.shade(rays, sun, mode=qmode, hits=True, status=True)
    hspx, _, hshits, hsstat, _ = p.host.shade(rays, sun, mode=qmode, hits=True, status=True)
    assert np.array_equal(bits(spx), bits(hspx))
    assert shits.tobytes() == hshits.tobytes() and sstat.tobytes() == hsstat.tobytes()


@pytest.mark.parametrize("name", ["bunny_97x61_primary", "quad", "tri1"])
def test_upkeep_of_the_device_scene(gpu, pairs, name):
    """Scene shape, SAH cost and refit.  A fresh pair of scenes: the refit changes them."""
    import torch
    pkg = gpu
    cfg = configs.CONFIGS[name]
    _, basis, sun = view_of(name, "exact")
    p = Pair(pkg, name, 0)
    try:
        a, b = p.dev.info(), p.host.info()
        assert (a["depth"], a["stack_entries"], a["n_pairs"]) == (b["depth"], b["stack_entries"], b["n_pairs"])
        assert a["stack_entries"] == max(1, a["depth"])
        c1, c2 = p.dev.sah_cost(), p.dev.sah_cost()
        assert qc.dbits(c1) == qc.dbits(c2)
        qc.assert_cost(c1, pkg.build_bvh(p.mesh).nodes, name)               # bound: (n + 16) * 2^-52
        moved = rc.deform(p.mesh)
        d_tri = torch.from_numpy(moved.tri.reshape(-1).copy()).to("cuda:0")
        d_norm = torch.from_numpy(moved.norm.reshape(-1).copy()).to("cuda:0")
        p.dev.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
        p.host.refit_device(d_tri.data_ptr(), d_norm.data_ptr())
        W, H, mode = cfg["W"], cfg["H"], pkg.cfg_mode(cfg)
        px, rgb, st = p.dev.render(basis, sun, W, H, mode=mode)
        hpx, hrgb, hst = p.host.render(basis, sun, W, H, mode=mode)
        assert np.array_equal(bits(px), bits(hpx)) and np.array_equal(rgb, hrgb)
        assert (st["rays"], st["hits"]) == (hst["rays"], hst["hits"])
        # ... and the refit moved something: the same scene as a fresh one over the numpy-refitted tree
        fresh = pkg.Scene(moved, pkg.Bvh(rc.refit_nodes(p.bvh.nodes, p.bvh.prim, moved.tri), p.bvh.prim))
        fpx, _, _ = fresh.render(basis, sun, W, H, mode=mode)
        fresh.close()
        assert np.array_equal(bits(px), bits(fpx))
        qc.assert_cost(p.dev.sah_cost(), rc.refit_nodes(p.bvh.nodes, p.bvh.prim, moved.tri), name + " refitted")
    finally:
        p.close()


def test_device_scene_rejects_malformed_bvh(gpu):
    """The four corruptions of tests/test_gpu_scene.py on 64-B nodes: each is refused by the validator (a null
    scene and a message), none reaches a render kernel, and a correct scene made afterwards renders."""
    import torch
    pkg = gpu
    name = "proc_101"
    cfg = configs.CONFIGS[name]
    mesh, bvh, _ = pkg.prepare(cfg, f64=True)
    n = len(mesh)
    d_tri = torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_prim = torch.from_numpy(bvh.prim.astype(np.uint32).view(np.int32)).to("cuda:0")
    inner = np.flatnonzero(bvh.nodes[:, 6] == 0)
    leaves = np.flatnonzero(bvh.nodes[:, 6] != 0)
    bad = []
    n1 = bvh.nodes.copy(); n1[inner[3], 7] = n1.shape[0] + 5; bad.append((n1, "child index out of range"))
    n2 = bvh.nodes.copy(); n2[inner[5], 7] = n2[inner[4], 7]; bad.append((n2, "node reached twice"))
    n3 = bvh.nodes.copy(); n3[leaves[0], 6] = n + 1; bad.append((n3, "leaf range out of bounds"))
    n4 = bvh.nodes.copy(); n4[inner[2], 7] = 2 ** 40; bad.append((n4, "child index out of range"))   # beyond 32 bits
    for nodes, why in bad:
        d_nodes = torch.from_numpy(nodes.view(np.int64).reshape(-1).copy()).to("cuda:0")
        with pytest.raises(pkg.CeresError, match=why):
            pkg.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), nodes.shape[0], d_prim.data_ptr())
    d_nodes = torch.from_numpy(bvh.nodes.view(np.int64).reshape(-1).copy()).to("cuda:0")
    pr = bvh.prim.astype(np.uint32).copy(); pr[7] = n + 3
    with pytest.raises(pkg.CeresError, match="primitive index out of range"):
        pkg.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), bvh.nodes.shape[0],
                                  torch.from_numpy(pr.view(np.int32)).to("cuda:0").data_ptr())
    with pytest.raises(pkg.CeresError):                                         # nodes off 16-byte alignment
        pkg.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr() + 8, bvh.nodes.shape[0] - 1,
                                  d_prim.data_ptr())
    with pytest.raises(pkg.CeresError):
        pkg.Scene.from_device_f64(0, n, d_norm.data_ptr(), d_nodes.data_ptr(), bvh.nodes.shape[0], d_prim.data_ptr())
    good = pkg.Scene.from_device_f64(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), bvh.nodes.shape[0], d_prim.data_ptr())
    host = pkg.Scene(mesh, bvh)
    meta, basis, sun = view_of(name, "exact")
    px, rgb, st = good.render(basis, sun, cfg["W"], cfg["H"], mode=pkg.cfg_mode(cfg))
    hpx, _, _ = host.render(basis, sun, cfg["W"], cfg["H"], mode=pkg.cfg_mode(cfg))
    good.close()
    host.close()
    assert np.array_equal(bits(px), bits(hpx))
    assert (st["rays"], st["hits"]) == (meta["exact"]["rays"], meta["exact"]["hits"])
    assert hashlib.sha256(pkg.ppm(cfg["W"], cfg["H"], rgb)).hexdigest() == meta["ppm_sha256"]["exact"]


@pytest.mark.parametrize("flag", ["", "--exact"])
def test_cli_double_gpu_bvh_writes_the_same_ppm(gpu, tmp_path, flag):
    """./render --double --gpu-bvh: the GPU double builder behind the CLI; the same bytes as the host build."""
    pkg = gpu
    name = "bunny_97x61_primary"
    meta = json.load(open(os.path.join(F64, name + ".json")))
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"
    args = configs.cli_args(configs.CONFIGS[name]) + ["--double"] + ([flag] if flag else [])
    ra = subprocess.run([pkg.CLI_PATH] + args + ["--gpu-bvh", "-o", str(a)], capture_output=True, text=True, timeout=120)
    rb = subprocess.run([pkg.CLI_PATH] + args + ["-o", str(b)], capture_output=True, text=True, timeout=120)
    assert ra.returncode == 0, ra.stderr
    assert rb.returncode == 0, rb.stderr
    assert "Building BVH ( using BinnedSahBuilder on the GPU )" in ra.stdout
    assert "on the GPU" not in rb.stdout
    assert a.read_bytes() == b.read_bytes()
    assert hashlib.sha256(a.read_bytes()).hexdigest() == meta["ppm_sha256"]["exact" if flag else "ref"]
