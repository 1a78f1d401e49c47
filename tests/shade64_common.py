"""Shared pieces of the shaded-ray-query tests on double scenes (test_shade_cpu_f64.py,
test_gpu_shade_f64.py): the checks both the CPU path and the GPU path must pass.  Each takes the
scene's own callables, `shade(rays, sun, mode, **outputs)`, `render(basis, sun, W, H, mode)` and
`trace(rays, mode, closest, occluded)`, and compares bit for bit or byte for byte -- no tolerance
anywhere.  The oracle is the reference's own render<double> frame (tests/golden/f64/): fed a view's
primary rays, a shaded ray query must return that framebuffer."""
import functools
import gzip
import hashlib
import os

import numpy as np

import trace64_common as t64
import trace_common as tc
from conftest import import_package

D = np.float64
# tri1 (the root is a leaf), quad (one step, no stack), degenerate, proc_101, bunny_1x1 (one ray: 63
# idle lanes), dragon_333x217 (all-miss, all-hit and mixed wavefronts)
FRAME_FIXTURES = ["tri1", "quad", "degenerate", "proc_101", "bunny_1x1", "dragon_333x217"]
BUILDS = ["exact", "ref"]
OUTPUTS = ("pixels", "rgb8", "hits", "status")
ALL = dict(pixels=True, rgb8=True, hits=True, status=True)
# what the dragon's records give (both builds): 64-ray groups all-miss / all-hit / mixed, a tail of 5
# rays, and the counts of status 0 / 1 / 2
DRAGON_GROUPS = (864, 2, 263)
DRAGON_STATUS = (63573, 4165, 4523)


def arith_of(build):
    return 1 if build == "ref" else 0


def mode_of(pkg, build):
    return pkg.MODE_FMA if build == "ref" else 0


def pixel_bytes(px):
    """Double pixels as bytes with every NaN mapped to one canonical NaN: x86 and gfx950 differ in the
    sign / payload of a generated NaN; the NaN positions still have to match (outputs_equal)."""
    a = np.array(px, D)
    a[np.isnan(a)] = D(np.nan)
    return a.tobytes()


def outputs_equal(a, b):
    """(pixels, rgb8, hits, status) of two paths: byte for byte, NaNs canonical and in the same places."""
    return (a[0].dtype == b[0].dtype == D and pixel_bytes(a[0]) == pixel_bytes(b[0])
            and np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and a[1].tobytes() == b[1].tobytes()
            and t64.hits_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))


def wavefront_kinds(status):
    """How many groups of 64 consecutive rays are all misses, all hits, and mixed."""
    hit = status != 0
    n = len(hit) // 64 * 64
    per = hit[:n].reshape(-1, 64).sum(axis=1)
    return int((per == 0).sum()), int((per == 64).sum()), int(((per > 0) & (per < 64)).sum())


def exact_ppm(name):
    with open(os.path.join(t64.F64_DIR, name + ".exact.ppm.gz"), "rb") as f:
        return gzip.decompress(f.read())


def check_camera_rays(pkg, name):
    """ceres_camera_rays_f64 in exact arithmetic == the numpy camera_rays64, bit for bit."""
    cfg, _, _, basis, _, _, _ = t64.fixture(name)
    W, H = cfg["W"], cfg["H"]
    a = pkg.camera_rays64(basis, W, H)
    b = pkg.camera_rays64_native(basis, W, H, pkg.ARITH_EXACT)
    assert a.dtype == b.dtype == D and a.shape == b.shape == (W * H, 8) and a.tobytes() == b.tobytes(), name


def check_camera_rays_fma(pkg, name):
    """... and in the reference CMake build's arithmetic == the exact rational fma (64 x 48 views)."""
    cfg, _, _, basis, _, _, _ = t64.fixture(name, "ref")
    W, H = cfg["W"], cfg["H"]
    assert W * H <= 64 * 48
    a = pkg.camera_rays64(basis, W, H, arith=pkg.ARITH_FMA)
    assert a.tobytes() == pkg.camera_rays64_native(basis, W, H, pkg.ARITH_FMA).tobytes()
    assert a.dtype == D and a.tobytes() == t64.camera_rays64_fma(basis, W, H).tobytes(), name


def check_frame_against_fixture(pkg, shade, render, trace, name, build):
    """The fixture's view through its own primary rays, in the contraction-free build ("exact") or the
    reference CMake build's arithmetic ("ref"): pixels == the reference's recorded rgb and render()'s
    framebuffer, the PPM == the reference's, rays / hits == the recorded pair, hits == the ray query's
    and the records', status == the records' shadow flags."""
    cfg, mesh, bvh, basis, sun, meta, rec = t64.fixture(name, build)
    W, H = cfg["W"], cfg["H"]
    n = W * H
    mode = mode_of(pkg, build)
    rays = pkg.camera_rays64(basis, W, H, arith=arith_of(build))
    px, rgb, hits, status, st = shade(rays, sun, mode, **ALL)
    assert px.dtype == D and px.shape == (n, 3) and rgb.shape == (n, 3) and status.shape == (n,)
    assert hits.dtype == pkg.HIT64_DTYPE
    p = rec["pixel"].astype(np.int64)
    assert len(p) == n
    assert np.array_equal(px[p].view(np.uint64), rec["rgb"].reshape(-1, 3).view(np.uint64)), (name, build)
    rpx, _, rst = render(basis, sun, W, H, mode)
    assert np.array_equal(px.reshape(-1).view(np.uint64), np.asarray(rpx, D).view(np.uint64)), (name, build)
    body = pkg.ppm(W, H, rgb.reshape(H, W, 3)[::-1])
    assert hashlib.sha256(body).hexdigest() == meta["ppm_sha256"][build], (name, build)
    if build == "exact":
        assert body == exact_ppm(name), name
    assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"]) == (rst["rays"], rst["hits"]), (name, build)
    n_hit, n_shadow = int((status != 0).sum()), int((status == 2).sum())
    assert (st["primary_rays"], st["shadow_rays"]) == (n, n_hit) and st["rays"] == n + n_hit and st["hits"] == n_hit + n_shadow
    h2, _, _ = trace(rays, mode, True, False)
    assert t64.hits_equal(hits, h2) and t64.hits_equal(hits, t64.expected_hits(pkg, rec, n)), (name, build)
    t64.assert_misses_are_zero(hits)
    assert np.array_equal(status[p] == 2, rec["shadow"] == 1), (name, build)
    assert np.array_equal(status[p] == 0, rec["prim"] < 0), (name, build)
    assert not px[status != 1].view(np.uint64).any() and not rgb[status != 1].any(), (name, build)
    if name == t64.DRAGON:
        assert wavefront_kinds(status) == DRAGON_GROUPS and n % 64 == 5, wavefront_kinds(status)
        assert tuple(np.bincount(status, minlength=3)) == DRAGON_STATUS
    if name == "bunny_1x1":
        assert n == 1
    return status, st


# ---------------------------------------------------------------- rays no camera makes

def tiny_sun(name):
    """shade_common.tiny_sun's recipe on the double mesh, kept in float64: the sun far beyond the edge
    opposite p0 of the first triangle, 1e-4 rad above its plane on the +n side, so that a shadow ray
    crosses the plane again 0.1 length units from its hit point -- inside the triangle for most hits
    (in shadow), past its outline for hits near the edge (lit)."""
    _, mesh, _, _, _, _, _ = t64.fixture(name)
    tr = np.asarray(mesh.tri[0], D)
    p0, e1, e2, n = tr[0:3], tr[3:6], tr[6:9], tr[9:12]
    n = n / np.linalg.norm(n)
    centre = p0 + (e2 - e1) / 3
    along = (p0 - e1 + p0 + e2) / 2 - p0                               # from p0 towards the opposite edge
    size = np.linalg.norm(along)
    return centre + 40 * along + n * size * 40 * 1e-4


LATTICE_SUN = np.asarray([-3, 9, 2.5], D)                             # shade_common.LATTICE_SUN
# the sets of the composition test and of GPU against CPU, with their status counts (miss, lit, in
# shadow) in exact arithmetic on the CPU path
COMPOSITION_SETS = ["adversarial", "tri1_tiny", "quad_tiny"]
PARITY_SETS = COMPOSITION_SETS + ["lattice", "proc33_brute"]
EXACT_COUNTS = {"adversarial": (3694, 122, 283), "tri1_tiny": (325, 10, 22), "quad_tiny": (298, 17, 42),
                "lattice": (3135, 649, 312), "proc33_brute": (914, 615, 108)}
FLOORED_SETS = ("adversarial", "proc33_brute")                        # at least 50 rays of each status


@functools.lru_cache(maxsize=None)
def ray_set(label, build="exact"):
    """(mesh, bvh, rays, sun) of a set, the scene prepared in the build's arithmetic; the sun is the
    same finite point in both."""
    pkg = import_package()
    if label == "adversarial":
        return t64.fixture(t64.DRAGON, build)[1:3] + (t64.adversarial_rays(), t64.fixture(t64.DRAGON)[4])
    if label.endswith("_tiny"):
        name = label[:-5]
        return t64.fixture(name, build)[1:3] + (t64.tiny_tree_rays(name), tiny_sun(name))
    if label == "lattice":
        return t64.lattice64(build)[1:3] + (tc.lattice_rays().astype(D), LATTICE_SUN)
    assert label == "proc33_brute"
    sun = t64.fixture("proc_101")[4]
    if build == "exact":
        return t64.brute_scene("proc33") + (t64.brute_rays("proc33"), sun)
    mesh = pkg.proc_mesh_f64(33, arith_of(build))
    return mesh, pkg.build_bvh(mesh, arith_of(build)), t64.brute_rays("proc33"), sun


def compose(pkg, mesh, trace, rays, sun):
    """What a caller composes from the double ray queries in contraction-free numpy: closest hits ->
    shadow_rays64 -> occlusion -> status (0 miss, 1 lit, 2 in shadow)."""
    hits, _, _ = trace(rays, 0, True, False)
    with np.errstate(all="ignore"):
        srays, idx = pkg.shadow_rays64(mesh, hits, sun)
    status = np.zeros(len(rays), np.uint8)
    if len(idx):
        _, occ, _ = trace(srays, 0, False, True)
        status[idx] = 1 + occ
    return hits, status


def check_composition(pkg, shade, trace, label):
    """shade == the composition of the ray queries (exact arithmetic): hits byte for byte, the same
    status, pixels 0 wherever status != 1 and something else wherever it is 1 (ambient light alone is
    0.1, 0, 0.16), the counters' formula, and all three status values in the recorded numbers."""
    mesh, _, rays, sun = ray_set(label)
    assert np.isfinite(sun).all() and sun.dtype == D
    rays = np.array(rays)
    px, rgb, hits, status, st = shade(rays, sun, 0, **ALL)
    exp_hits, exp_status = compose(pkg, mesh, trace, rays, sun)
    assert t64.hits_equal(hits, exp_hits), label
    assert np.array_equal(status, exp_status), (label, np.flatnonzero(status != exp_status)[:8])
    assert not px[status != 1].view(np.uint64).any() and not rgb[status != 1].any(), label
    assert px[status == 1].view(np.uint64).any(axis=1).all(), label
    n_hit = int((status != 0).sum())
    assert (st["rays"], st["hits"]) == (len(rays) + n_hit, n_hit + int((status == 2).sum())), label
    assert (st["primary_rays"], st["shadow_rays"]) == (len(rays), n_hit), label
    assert tuple(np.bincount(status, minlength=3)) == EXACT_COUNTS[label], (label, np.bincount(status, minlength=3))


def check_parity_set_input(label, build, status):
    """What keeps the GPU-against-CPU comparison from being vacuous, on the CPU path's status."""
    count = np.bincount(status, minlength=3)
    assert count[1] > 0, (label, build, count)
    if label in FLOORED_SETS:
        assert count.min() >= 50, (label, build, count)
    if build == "exact":
        assert tuple(count) == EXACT_COUNTS[label], (label, count)
