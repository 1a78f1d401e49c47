"""Shared pieces of the shaded-ray-query tests (test_shade_cpu.py, test_gpu_shade.py): the checks both
the CPU path and the GPU path must pass.  Each takes the scene's own callables,
`shade(rays, sun, mode, **outputs)` and `render(basis, sun, W, H, mode)`, and compares bit for bit or
byte for byte -- no tolerance anywhere.  The oracle is the reference's own frame: fed a view's primary
rays, a shaded ray query must return render()'s framebuffer."""
import numpy as np

import trace_common as tc
from conftest import import_package, load_golden


def shaded_fixtures():
    """CLOSEST_FIXTURES whose config renders shadows and shading (not primary-only)."""
    pkg = import_package()
    return [n for n in tc.CLOSEST_FIXTURES if pkg.configs.CONFIGS[n]["mode"] != "primary"]


def pixel_bytes(px):
    """Float pixels as bytes with every NaN mapped to one canonical NaN: x86 and gfx950 differ in the
    sign / payload of a generated NaN; the NaN positions still have to match."""
    a = np.array(px, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def check_frame_against_fixture(pkg, shade, render, trace, name, arith):
    """The fixture's view through its own primary rays, in the exact (arith 0) or the reference CMake
    build's arithmetic: pixels == render()'s floats, the PPM == the reference's file, rays / hits ==
    the recorded pair, hits == the ray query's, status == the records' shadow flags."""
    cfg, mesh, bvh, basis, sun, meta, rec = tc.fixture(name, arith)
    W, H = cfg["W"], cfg["H"]
    build = "ref" if arith else "exact"
    mode = tc.mode_of(pkg, name) | (pkg.MODE_FMA if arith else 0)
    rays = pkg.camera_rays(basis, W, H, arith=arith)
    px, rgb, hits, status, st = shade(rays, sun, mode, pixels=True, rgb8=True, hits=True, status=True)
    rpx, _, rst = render(basis, sun, W, H, mode)
    assert px.shape == (W * H, 3) and rgb.shape == (W * H, 3) and status.shape == (W * H,)
    assert np.array_equal(px.reshape(-1).view(np.uint32), np.asarray(rpx, np.float32).view(np.uint32)), (name, build)
    ppm = load_golden(name)[2]
    assert pkg.ppm(W, H, rgb.reshape(H, W, 3)[::-1]) == ppm[build], (name, build)
    assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"]) == (rst["rays"], rst["hits"]), (name, build)
    assert st["primary_rays"] == W * H and st["shadow_rays"] == int((status != 0).sum()) == st["rays"] - W * H
    assert st["hits"] == int((status != 0).sum() + (status == 2).sum())
    h2, _, _ = trace(rays, mode, True, False)
    assert tc.hits_equal(hits, h2), (name, build)
    assert np.array_equal(status == 0, hits["prim"] < 0), (name, build)
    if not arith:                                                     # the records are the exact build's
        p = rec["pixel"]
        assert np.array_equal(status[p] == 2, rec["shadow"] == 1), name
        assert np.array_equal(status[p] == 0, rec["prim"] < 0), name
    assert not px[status != 1].view(np.uint32).any() and not rgb[status != 1].any(), (name, build)
    return status, st


def compose(pkg, mesh, trace, rays, sun, mode):
    """What a caller composes from the ray queries, in float32 numpy (contraction-free): closest hits ->
    shadow_rays -> occlusion -> status (0 miss, 1 lit, 2 in shadow)."""
    hits, _, _ = trace(rays, mode, True, False)
    with np.errstate(all="ignore"):
        srays, idx = pkg.shadow_rays(mesh, hits, sun)
    status = np.zeros(len(rays), np.uint8)
    if len(idx):
        _, occ, _ = trace(srays, mode, False, True)
        status[idx] = 1 + occ
    return hits, status


def check_composition(pkg, mesh, shade, trace, rays, sun, mode=0):
    """shade == the composition of the ray queries: hits byte for byte, the same status, pixels 0
    wherever status != 1 and something else wherever it is 1 (ambient light alone is 0.1, 0, 0.16)."""
    px, rgb, hits, status, st = shade(rays, sun, mode, pixels=True, rgb8=True, hits=True, status=True)
    exp_hits, exp_status = compose(pkg, mesh, trace, rays, sun, mode)
    assert tc.hits_equal(hits, exp_hits)
    assert np.array_equal(status, exp_status), np.flatnonzero(status != exp_status)[:8]
    assert not px[status != 1].view(np.uint32).any() and not rgb[status != 1].any()
    assert px[status == 1].view(np.uint32).any(axis=1).all()
    n_hit = int((status != 0).sum())
    assert (st["rays"], st["hits"]) == (len(rays) + n_hit, n_hit + int((status == 2).sum()))
    assert (st["primary_rays"], st["shadow_rays"]) == (len(rays), n_hit)
    return px, rgb, hits, status


def tiny_sun(name):
    """The sun of a smallest-tree set.  tri1 is ONE triangle: its only occluder is itself, met when the
    sun is on the side the hit point's offset (-0.00001 n) points away from.  So the sun sits far beyond
    the edge opposite p0 of the fixture's first triangle, 1e-4 rad above its plane on the +n side: a
    shadow ray crosses the plane again 0.00001 / 1e-4 = 0.1 length units from its hit point towards that
    edge -- still inside the triangle for most hits (in shadow), past its outline for hits near the edge
    (lit).  The composition test asserts that both occur."""
    _, mesh, _, _, _, _, _ = tc.fixture(name)
    tr = mesh.tri[0].astype(np.float64)
    p0, e1, e2, n = tr[0:3], tr[3:6], tr[6:9], tr[9:12]
    n = n / np.linalg.norm(n)
    centre = p0 + (e2 - e1) / 3
    along = (p0 - e1 + p0 + e2) / 2 - p0                               # from p0 towards the opposite edge
    size = np.linalg.norm(along)
    return (centre + 40 * along + n * size * 40 * 1e-4).astype(np.float32)


def composition_sets():
    """(fixture, rays, sun) of the composition test: the adversarial set under the dragon's own sun and
    the two smallest-tree sets."""
    out = [(tc.DRAGON, tc.adversarial_rays(), tc.fixture(tc.DRAGON)[4])]
    for name in tc.TINY_FIXTURES:
        out.append((name, tc.tiny_tree_rays(name), tiny_sun(name)))
    return out


LATTICE_SUN = np.asarray([-3, 9, 2.5], np.float32)                     # beside and a little above the layers z = 0, 1, 2
PARITY_SETS = ["adversarial", "tri1_tiny", "quad_tiny", "lattice", "lattice_octants", "proc300_window"]
FLOORED_SETS = ("adversarial", "proc300_window")                      # at least 50 rays of each status


def parity_set(label, arith=0):
    """(mesh, bvh, rays, sun) of a GPU-against-CPU set, the scene prepared in the given arithmetic; the
    sun is the same finite point in every arithmetic (checked on the CPU path: test_shade_cpu.py)."""
    pkg = import_package()
    if label == "adversarial":
        return tc.fixture(tc.DRAGON, arith)[1:3] + (tc.adversarial_rays(), tc.fixture(tc.DRAGON)[4])
    if label.endswith("_tiny"):
        name = label[:-5]
        return tc.fixture(name, arith)[1:3] + (tc.tiny_tree_rays(name), tiny_sun(name))
    if label.startswith("lattice"):
        rays = tc.lattice_rays()
        if label == "lattice_octants":
            rays = np.ascontiguousarray(rays[tc.lattice_octant_order(rays)])
        return tc.lattice(arith)[1:3] + (rays, LATTICE_SUN)
    assert label == "proc300_window"
    cfg, mesh, bvh, _ = tc.proc300(arith)
    return mesh, bvh, tc.proc300_window_rays(), np.asarray(cfg["sun"], np.float32)


def check_parity_set_input(label, status):
    """What keeps the GPU-against-CPU comparison from being vacuous, on the CPU path's status."""
    count = np.bincount(status, minlength=3)
    assert count[1] > 0, (label, count)
    if label in FLOORED_SETS:
        assert count.min() >= 50, (label, count)


def outputs_equal(a, b):
    """(pixels, rgb8, hits, status) of two paths: byte for byte, NaNs canonical."""
    return (pixel_bytes(a[0]) == pixel_bytes(b[0]) and np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
            and a[1].tobytes() == b[1].tobytes() and tc.hits_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))
