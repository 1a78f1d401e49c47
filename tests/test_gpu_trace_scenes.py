"""Ray queries and hit records on the two scene flavours the other trace tests never build: scenes laid
out on the GPU (build_bvh_device + Scene.from_device: scene_device.hip's relayout, with its own record
numbering, its own orig[] and BVH4 and its own stack bounds) and first-order scenes (Scene(...,
first_order=True): the shadow BVH4's children reordered by order_shadow_bvh4).  Both are otherwise
tested through rendered frames only -- one camera's primary rays, one sun's shadow rays.  Here they
answer the stored caller rays of tests/golden/rays/ (every octant, windows, non-finite rays, exact
ties) and the fixtures' recorded pixels, against the reference's own answers, bit for bit; and the
device relayout's BVH4 stack bound is compared with the restatement of test_gpu_shadow_stack.py."""
import functools

import numpy as np
import pytest

import trace_common as tc
from test_gpu_scene import device_scene
from test_gpu_shadow_stack import _bounds

pytestmark = pytest.mark.gpu

DEVICE_CLOSEST = ["tri1", "quad", "dupleaf", "degenerate", "proc_101", tc.DRAGON]
RECORD_FIXTURES = [tc.DRAGON, "dupleaf", "tri1", "proc_101"]
BOUND_SCENES = ["dragon_1080", "bunny_1080", "proc_101"]


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@functools.lru_cache(maxsize=None)
def _arrays(pkg, name, arith):
    """((scene key), mesh, bvh) of a ray set's or a config's scene: one scene per mesh and arithmetic."""
    if name in tc.RAY_SETS:
        cfg = tc.ray_set_config(name)
        mesh, bvh = tc.ray_set_scene(name, arith)
    else:
        cfg = pkg.configs.CONFIGS[name]
        mesh, bvh = tc.fixture(name, arith)[1:3] if name in tc.CLOSEST_FIXTURES else pkg.prepare(cfg, arith=arith)[0:2]
    return (cfg["obj"], cfg["proc"], cfg["rotate"], arith), mesh, bvh


@pytest.fixture(scope="module")
def scenes(gpu):
    """device(name, arith, stats) -> a scene built and laid out on the GPU; first(name, arith) -> a
    first-order scene; host(name, arith) -> the plain host-built scene.  Each created once."""
    import torch
    cache, keep = {}, {}

    class Get:
        def device(self, name, arith=0, stats=False):
            key, mesh, bvh = _arrays(gpu, name, arith)
            if key not in keep:
                keep[key] = (torch.from_numpy(mesh.tri.reshape(-1).copy()).to("cuda:0"),
                             torch.from_numpy(mesh.norm.reshape(-1).copy()).to("cuda:0"))
            if ("device", key, stats) not in cache:
                d_tri, d_norm = keep[key]
                scene, m = device_scene(gpu, d_tri.data_ptr(), len(mesh), d_norm.data_ptr(), arith, stats=stats)
                cache["device", key, stats] = scene
                assert m == bvh.nodes.shape[0], name                  # as many nodes as the host builder's tree
            return cache["device", key, stats]

        def first(self, name, arith=0):
            key, mesh, bvh = _arrays(gpu, name, arith)
            if ("first", key) not in cache:
                cache["first", key] = gpu.Scene(mesh, bvh, first_order=True)
            return cache["first", key]

        def host(self, name, arith=0):
            key, mesh, bvh = _arrays(gpu, name, arith)
            if ("host", key) not in cache:
                cache["host", key] = gpu.Scene(mesh, bvh)
            return cache["host", key]

    yield Get()
    for s in cache.values():
        s.close()
    keep.clear()


def tracer(scene):
    return lambda rays, mode, closest, occluded: scene.trace(rays, mode=mode, closest=closest, occluded=occluded)


# ---------------------------------------------------------------- scenes laid out on the GPU

@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_device_scene_caller_rays_equal_the_reference_traverser(gpu, scenes, name, variant):
    """Every stored ray set on the device-built scene: the production kernels with both queries,
    closest only and occluded only, and the stats kernels with the reference's summed Statistics."""
    arith = tc.variant_mode(gpu, variant)[1]
    prod, st = tracer(scenes.device(name, arith)), tracer(scenes.device(name, arith, stats=True))
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False)
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False, occluded=False)
    tc.check_against_ray_fixture(gpu, prod, name, variant, stats=False, closest=False)
    tc.check_against_ray_fixture(gpu, st, name, variant, stats=True)


@pytest.mark.parametrize("name", DEVICE_CLOSEST)
def test_device_scene_closest_hit_equals_reference_records(gpu, scenes, name):
    """tri1: the root is a leaf; dupleaf: leaves above 31 triangles, which the device relayout hands
    to the host's BVH4 builder.  Stats scene: the reference's primary-ray Statistics."""
    _, hits = tc.check_closest_against_fixture(gpu, tracer(scenes.device(name, stats=True)), name)
    _, hits2 = tc.check_closest_against_fixture(gpu, tracer(scenes.device(name)), name, check_stats=False)
    assert tc.hits_equal(hits, hits2)


@pytest.mark.parametrize("name", DEVICE_CLOSEST)
def test_device_scene_occlusion_equals_reference_shadow_flags(gpu, scenes, name):
    if name not in tc.OCCLUSION_FIXTURES:                             # degenerate: rendered in full mode all the same
        assert gpu.configs.CONFIGS[name]["mode"] == "full"
    tc.check_occlusion_against_fixture(gpu, tracer(scenes.device(name, stats=True)), name)
    tc.check_occlusion_against_fixture(gpu, tracer(scenes.device(name)), name)


# ---------------------------------------------------------------- first-order scenes

@pytest.mark.parametrize("name", tc.OCCLUSION_FIXTURES)
def test_first_order_occlusion_equals_reference_shadow_flags(gpu, scenes, name):
    tc.check_occlusion_against_fixture(gpu, tracer(scenes.first(name)), name)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_first_order_caller_rays_equal_the_reference_traverser(gpu, scenes, name, variant):
    """The occlusion walk reads the reordered BVH4: occluded only, and both queries in one launch."""
    sc = tracer(scenes.first(name, tc.variant_mode(gpu, variant)[1]))
    tc.check_against_ray_fixture(gpu, sc, name, variant, stats=False, closest=False)
    tc.check_against_ray_fixture(gpu, sc, name, variant, stats=False)


# ---------------------------------------------------------------- hit records

@pytest.mark.parametrize("flavour", ["device", "first"])
@pytest.mark.parametrize("name", RECORD_FIXTURES)
def test_records_equal_reference_records(gpu, scenes, name, flavour):
    """scene.records at the fixture's recorded pixels: {prim, t, u, v, shadow} of the contraction-free
    reference, bit for bit -- the device relayout's orig[] read directly, not through shading."""
    cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(name)
    scene = scenes.device(name) if flavour == "device" else scenes.first(name)
    prim, tuv, sh, _ = scene.records(basis, sun, cfg["W"], cfg["H"], mode=gpu.cfg_mode(cfg))
    pix = rec["pixel"].astype(np.int64)
    assert np.array_equal(prim[pix], rec["prim"]), name
    assert np.array_equal(sh[pix], rec["shadow"]), name
    hit = rec["prim"] >= 0
    assert hit.any()
    for k, key in enumerate(("t", "u", "v")):
        assert tc.same_bits(tuv[pix][hit, k], rec[key][hit]), (name, key)


# ---------------------------------------------------------------- the device relayout's stack bounds

@pytest.mark.parametrize("name", BOUND_SCENES)
def test_device_scene_stack_bound_matches_restatement(gpu, scenes, name):
    """The BVH4 the device relayout builds (k_nodes4) needs the stack the restatement of
    test_gpu_shadow_stack.py computes from the BVH2 alone; a device-built scene is never reordered,
    so both walks use the nearest-first bound."""
    _, mesh, bvh = _arrays(gpu, name, 0)
    near, _ = _bounds(bvh.nodes)
    info = scenes.device(name).info()
    assert info["shadow_stack_nearest"] == near, name
    assert info["shadow_stack_first"] == info["shadow_stack_nearest"], name
    host = scenes.host(name).info()
    assert (info["depth"], info["stack_entries"], info["n_pairs"]) == (host["depth"], host["stack_entries"], host["n_pairs"])


def test_device_scene_stack_bound_equals_host_scene_on_dupleaf(gpu, scenes):
    """dupleaf's leaves of 40 and 130 triangles become piece nodes, which the restatement does not
    model: this compares two builds of the product (device relayout against host relayout), not an
    independent restatement."""
    a, b = scenes.device("dupleaf").info(), scenes.host("dupleaf").info()
    assert a["shadow_stack_nearest"] == b["shadow_stack_nearest"] >= 1
    assert a["shadow_stack_first"] == b["shadow_stack_first"]
