"""The 24- and 32-bit-stack kernels on small scenes (render_hip.hip stack_width, Stk24 / uint32_t*).

The width of an LDS stack entry follows the scene's record count: 2 bytes below 2^16 sibling pairs
and BVH4 records, 3 below 2^24, else 4.  Every launcher -- ceres_fused in all its flavours,
ceres_trace_rays_k, ceres_shade_rays_k -- dispatches on it, so a third of the kernel instantiations
sit behind each value, and only scenes of tens of millions of triangles reach the widest by
themselves.  CERES_DEBUG_STACK_WIDTH=3|4, read when a scene is created, widens that scene's entries
(never narrows them); Scene.stack_width() reports what the launches use.

The entry width changes nothing a walk decides, so the bar is equality: every output byte and every
counter of a widened scene equals the natural-width scene's, which the other suites pin to the
reference (fixtures, the reference traverser, the CPU path).  proc_300 (178,802 triangles, 93,876
pairs: naturally 24-bit, L2-resident, so its batches compact) is also held to its own fixture here,
and at width 4 its stack entries exceed 65535: a 32-bit path that lost the upper half shows there.

What shows that a launch took the intended instantiation: stack_width(), info()["n_pairs"],
compact_order() (the batch compacted), its tpw and entry_nodes()["used"] (the 16-bit-only kernels).

Stats scenes here are created with first_order=True.  The child order of a host-made scene's BVH4
records is chosen by the LDS its stacks cost (lds_limits_waves), which the width changes, and the
shadow walk's node and triangle counters depend on that order (the images, records and hit counts do
not).  Measured with default flags, proc_101's own view at 333x217: widths 2 and 3 keep the build
order (1,732,802 node pairs, 373,034 triangle tests), width 4 crosses the LDS threshold and orders
the records (1,732,526 and 372,981) -- the counts a first_order=True scene gives at every width.
With the flag both widths hold the same records, so the counters must be equal too."""
import contextlib
import hashlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import load_golden, ppm_budget_ok

import configs
import cull_fill_model as M
import tile_compact_model as C
import trace_common as T

pytestmark = pytest.mark.gpu

ENV = "CERES_DEBUG_STACK_WIDTH"
NATURAL = {"proc_101": 2, "proc_300": 3, "dupleaf": 2, "tri1": 2, "dragon_333x217": 2}
CASES = [("proc_101", 2), ("proc_101", 3), ("proc_101", 4), ("proc_300", 3), ("proc_300", 4), ("dupleaf", 3),
         ("dupleaf", 4), ("tri1", 4)]
WIDE = [c for c in CASES if c[1] != NATURAL[c[0]]]
SIZES = [(136, 72), (333, 217)]
# 16 <-> 24 bits: prefixes of proc_mesh(260)'s 134,162 triangles (ARITH_FMA), see the threshold test
PREFIX_LAST_16 = 121765
PREFIX_FIRST_24 = 121767


@contextlib.contextmanager
def forced(width):
    """CERES_DEBUG_STACK_WIDTH while a scene is created (None: unset); the environment is restored."""
    old = os.environ.pop(ENV, None)
    if width is not None:
        os.environ[ENV] = str(width)
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


class _Env:
    """One config's meshes and BVHs in both arithmetics and its scenes by (width, arith, kind)."""

    def __init__(self, pkg, name):
        self.pkg, self.name = pkg, name
        self.cfg = configs.CONFIGS[name]
        self.prep = {a: pkg.prepare(self.cfg, arith=a) for a in (pkg.ARITH_EXACT, pkg.ARITH_FMA)}
        self.mesh, self.bvh, self.cam = self.prep[pkg.ARITH_FMA]
        self.root = M.root_box(self.mesh.tri)
        self.sun = np.asarray(self.cfg["sun"], np.float32)
        self.full = pkg.MODE_FULL | pkg.MODE_FMA
        self.scenes, self.refs, self.cams = {}, {}, {}

    def scene(self, width=None, arith=None, kind="prod", mod=None):
        """kind: prod | first (first_order) | stats (stats + first_order); mod: another build of the package."""
        pkg = self.pkg
        arith = pkg.ARITH_FMA if arith is None else arith
        width = NATURAL[self.name] if width is None else width
        key = (width, arith, kind, mod)
        if key not in self.scenes:
            mesh, bvh, _ = self.prep[arith]
            with forced(width):
                sc = (mod or pkg).Scene(mesh, bvh, stats=kind == "stats", first_order=kind != "prod")
            assert sc.stack_width() == width, "the scene's launches do not use the asked width"
            self.scenes[key] = sc
        return self.scenes[key]

    def views(self, W, H):
        """tile_compact_model.cameras' odd / gone / centre / inside and the config's own camera."""
        if (W, H) not in self.cams:
            v = C.cameras(self.pkg, self.root, W, H)
            v["cfg"] = np.asarray(self.cam.basis(W, H), np.float32)
            self.cams[W, H] = v
        return self.cams[W, H]

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def envs(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    assert ENV not in os.environ, "the suite runs with the hook unset"
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Env(pkg, name)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _call(e, scene, b12, W, H, tiling=None, rows=None, mode=None):
    """One batch call into patterned buffers -> (float bytes, RGB8 bytes, 8 counters); guards checked."""
    import torch
    F, rows = len(b12), H if rows is None else rows
    n = 3 * F * rows * W
    px = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    scene.render_batch_device(b12, np.repeat(e.sun[None], F, 0), W, H, mode=e.full if mode is None else mode, tiling=tiling,
                              d_pixels=px.data_ptr(), d_rgb8=rgb.data_ptr(), d_counters=cnt.data_ptr())
    torch.cuda.synchronize()
    px, rgb = px.cpu().numpy(), rgb.cpu().numpy()
    assert (px[4 * n:] == 0xA5).all() and (rgb[n:] == 0xA5).all(), "a store behind the buffers"
    return px[:4 * n].reshape(F, -1), rgb[:n].reshape(F, -1), [int(x) for x in cnt.cpu().numpy()]


def _ref(e, b, W, H, tiling=None, rows=None, key=None, mode=None, arith=None):
    """The natural-width stats scene's one-frame launch of a view: computed once, shared, never changed."""
    key = (b.tobytes(), W, H, key, mode, arith)
    if key not in e.refs:
        px, rgb, c = _call(e, e.scene(None, arith, "stats"), b[None], W, H, tiling, rows, mode)
        assert c[6] == 0
        px.setflags(write=False)
        rgb.setflags(write=False)
        e.refs[key] = (px[0], rgb[0], c[:4])
    return e.refs[key]


def _parity(e, scene, b12, W, H, tiling=None, rows=None, key=None, mode=None, arith=None):
    """A batch against its frames one per launch on the stats scene (mode: e.full; arith: ARITH_FMA)."""
    px, rgb, c = _call(e, scene, b12, W, H, tiling, rows, mode)
    assert c[6] == 0, "the launch's error word"
    want = [0, 0, 0, 0]
    for f, b in enumerate(b12):
        rp, rr, rc = _ref(e, b, W, H, tiling, rows, key, mode, arith)
        assert np.array_equal(px[f], rp), f"float framebuffer of frame {f} differs"
        assert np.array_equal(rgb[f], rr), f"RGB8 body of frame {f} differs"
        want = [x + y for x, y in zip(want, rc)]
    assert c[:4] == want
    return px, rgb, c


def _same_frame(a, b, what, keys=("rays", "hits", "primary_rays", "shadow_rays")):
    (pa, ra, sa), (pb, rb, sb) = a, b
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), what + ": float pixels differ"
    assert np.array_equal(ra, rb), what + ": RGB8 differs"
    for k in keys:
        assert sa[k] == sb[k], (what, k)


def _check_batch_path(e, scene, width, robust=False):
    """What the latest batch launch must have taken: a compacted order wherever the scene culls (a root
    leaf has no root box to cull by), four tiles per wave, and entry nodes on 16-bit stacks only (and
    never with the robust slabs)."""
    order = scene.compact_order()
    if e.name == "tri1":
        assert order is None and not scene.entry_nodes()["used"]
        return
    assert order is not None, "the launch took the plain grid"
    assert order["tpw"] == 4
    assert scene.entry_nodes()["used"] == (width == 2 and not robust), "entry nodes: the 16-bit-stack kernels, and only they"


@pytest.mark.parametrize("name,width", CASES)
def test_hook_widens_and_is_kept_in_the_scene(envs, name, width, monkeypatch):
    """The width is read when the scene is made and kept: what the environment holds later changes
    nothing; values other than 3 and 4 are ignored (CASES' width 2 is such a value); it only widens."""
    e = envs(name)
    pkg = e.pkg
    sc = e.scene(width)
    assert e.scene().stack_width() == NATURAL[name]
    if name == "proc_300":
        assert sc.info()["n_pairs"] >= 1 << 16
    for junk in ("4", "2", "5", "3x", "", "-4", "0x4"):
        monkeypatch.setenv(ENV, junk)
        assert sc.stack_width() == width
        if junk != "4":
            with_junk = pkg.Scene(e.mesh, e.bvh)
            assert with_junk.stack_width() == NATURAL[name], junk
            with_junk.close()
    if name == "proc_300":
        monkeypatch.setenv(ENV, "3")
        narrow = pkg.Scene(e.mesh, e.bvh)
        assert narrow.stack_width() == 3
        narrow.close()
    monkeypatch.delenv(ENV)
    W, H = SIZES[0]
    b = e.views(W, H)["centre"]
    _same_frame(sc.render(b, e.sun, W, H, mode=e.full), e.scene().render(b, e.sun, W, H, mode=e.full), "after the variable is gone")


@pytest.mark.parametrize("kind", ["prod", "first"])
@pytest.mark.parametrize("name,width", CASES)
def test_solo_frames(envs, name, width, kind):
    """One-frame launches (the work-stealing kernel), exact and FMA arithmetic, fast and robust slabs, on
    a default scene and on a first_order=True one (steal_first): float pixels, RGB8, rays and hits."""
    e = envs(name)
    pkg = e.pkg
    for arith, fma in ((pkg.ARITH_EXACT, 0), (pkg.ARITH_FMA, pkg.MODE_FMA)):
        got, nat = e.scene(width, arith, kind), e.scene(None, arith, kind)
        for robust in (0, pkg.MODE_ROBUST):
            mode = pkg.MODE_FULL | fma | robust
            for W, H in SIZES:
                for view in ("cfg", "odd") if (W, H) == SIZES[1] else ("centre",):
                    b = e.views(W, H)[view]
                    _same_frame(got.render(b, e.sun, W, H, mode=mode), nat.render(b, e.sun, W, H, mode=mode),
                                f"{name} width {width} {kind} fma={fma} robust={robust} {W}x{H} {view}")


@pytest.mark.parametrize("width", [3, 4])
def test_proc_300_equals_its_fixture(envs, width):
    """proc_300's own frame against the reference's PPM and counts, both builds, at both widths."""
    e = envs("proc_300")
    pkg = e.pkg
    meta, _, _ = load_golden("proc_300")
    cfg = e.cfg
    W, H = cfg["W"], cfg["H"]
    for build, arith in (("exact", pkg.ARITH_EXACT), ("ref", pkg.ARITH_FMA)):
        sc = e.scene(width, arith)
        assert sc.info()["n_pairs"] >= 1 << 16
        bb = meta["ref_basis"] if build == "ref" else meta["basis"]
        bits = [int(h, 16) for h in bb["dir"] + bb["u"] + bb["v"]]
        basis = np.concatenate([np.asarray(cfg["eye"], np.float32), np.asarray(bits, np.uint32).view(np.float32)])
        _, rgb, st = sc.render(basis, cfg["sun"], W, H, mode=pkg.cfg_mode(cfg, arith))
        assert (st["rays"], st["hits"]) == (meta[build]["rays"], meta[build]["hits"]), build
        assert hashlib.sha256(pkg.ppm(W, H, rgb)).hexdigest() == meta["ppm_sha256"][build], build


@pytest.mark.parametrize("W,H,views", [(136, 72, ("odd", "gone", "centre", "inside")),
                                       (333, 217, ("inside", "gone", "odd", "cfg", "centre"))])
@pytest.mark.parametrize("name,width", CASES)
def test_batches_cull_and_compact(envs, name, width, W, H, views):
    """Batches whose launches cull and read a compacted order, exact and FMA, fast and robust, against
    one-frame launches of the natural-width stats scene (which never culls, compacts or enters below
    the root)."""
    e = envs(name)
    pkg = e.pkg
    v = e.views(W, H)
    b12 = np.stack([v[k] for k in views])
    for arith, fma in ((pkg.ARITH_EXACT, 0), (pkg.ARITH_FMA, pkg.MODE_FMA)):
        sc = e.scene(width, arith)
        if name == "proc_300":
            assert sc.info()["n_pairs"] >= 1 << 16
        for robust in (0, pkg.MODE_ROBUST):
            _parity(e, sc, b12, W, H, mode=pkg.MODE_FULL | fma | robust, arith=arith)
            _check_batch_path(e, sc, width, bool(robust))


def test_two_1080p_frames_at_24_bits_take_four_tiles_per_wave(envs):
    """16-bit-stack scenes take two tiles per wave at 1080p; the kernels compiled for two exist for
    them only, so the same scene with a wider stack must take four."""
    e = envs("proc_101")
    W, H = 1920, 1080
    v = e.views(W, H)
    b12 = np.stack([v["centre"], v["odd"]])
    _parity(e, e.scene(), b12, W, H)
    assert e.scene().compact_order()["tpw"] == 2
    sc = e.scene(3)
    _parity(e, sc, b12, W, H)
    _check_batch_path(e, sc, 3)


@pytest.mark.parametrize("name,width", WIDE + [("proc_300", 3)])
def test_band_and_row_block_tilings(envs, name, width):
    """ceres_tiling.bands (world 2, both ranks: frame f renders band (rank + f) mod 2) and a row-block
    tiling, against the natural-width stats scene rendering the same rows -- which are the whole
    frame's rows, cut out of its one-frame launch."""
    e = envs(name)
    pkg = e.pkg
    sc = e.scene(width)
    for W, H in SIZES:
        v = e.views(W, H)
        b12 = np.stack([v["odd"], v["gone"], v["centre"]])
        whole = [_ref(e, b, W, H) for b in b12]
        rb, world = (H + 1) // 2, 2
        for rank in range(world):
            px, rgb, c = _call(e, sc, b12, W, H, pkg.Tiling(rb, rank, world, 1), rb)
            assert c[6] == 0 and sc.compact_order() is None
            want = [0, 0, 0, 0]
            for f, b in enumerate(b12):
                band = (rank + f) % world
                rows = min(rb, H - band * rb)
                rp, rr, rc = _ref(e, b, W, H, pkg.Tiling(rb, band, world, 0), rows, key=("band", band))
                # float rows from the bottom up, local row k at k; RGB8 rows flipped (the PPM's order), local
                # row k at local_rows - 1 - k -- a last band shorter than rb ends at its slot's end
                assert np.array_equal(px[f][:12 * W * rows], rp) and np.array_equal(rgb[f][3 * W * (rb - rows):], rr), (rank, f)
                lo = band * rb
                assert np.array_equal(rp, whole[f][0][12 * W * lo:12 * W * (lo + rows)]), "the band is not the frame's rows"
                assert np.array_equal(rr, whole[f][1][3 * W * (H - lo - rows):3 * W * (H - lo)])
                want = [x + y for x, y in zip(want, rc)]
            assert c[:4] == want
        for rank, rows_of in enumerate(pkg.row_map(H, 16, 2)):
            t = pkg.Tiling(16, rank, 2, 0)
            px, rgb, _ = _parity(e, sc, b12, W, H, tiling=t, rows=len(rows_of), key=("rb", rank))
            assert sc.compact_order() is None
            for f in range(len(b12)):
                assert np.array_equal(rgb[f].reshape(-1, 3 * W), whole[f][1].reshape(H, 3 * W)[H - 1 - rows_of[::-1]])
                assert np.array_equal(px[f].reshape(-1, 12 * W), whole[f][0].reshape(H, 12 * W)[rows_of])


@pytest.mark.parametrize("name,width", CASES)
def test_qbvh4(envs, name, width):
    """The compressed shadow BVH4: the same bytes at every width, solo and batch; and proc_300 within the
    SURVEY section 7 budget against its exact frame, no occluded pixel turned lit (as test_gpu_qbvh.py)."""
    e = envs(name)
    pkg = e.pkg
    mode = e.full | pkg.MODE_QBVH4
    got, nat = e.scene(width), e.scene()
    for W, H in SIZES:
        v = e.views(W, H)
        for view in ("cfg", "centre"):
            _same_frame(got.render(v[view], e.sun, W, H, mode=mode), nat.render(v[view], e.sun, W, H, mode=mode),
                        f"{name} width {width} {W}x{H} {view}")
        b12 = np.stack([v["odd"], v["gone"], v["cfg"]])
        a, b = _call(e, got, b12, W, H, mode=mode), _call(e, nat, b12, W, H, mode=mode)
        assert a[2][6] == 0 and a[2][:4] == b[2][:4]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if name != "tri1":
            assert got.compact_order() is not None and got.compact_order()["tpw"] == 4
            assert not got.entry_nodes()["used"], "QBVH4 launches enter at the root"
    if name == "proc_300":
        W, H = SIZES[1]
        b = e.views(W, H)["cfg"]
        _, rgb_e, st_e = got.render(b, e.sun, W, H, mode=e.full)
        _, rgb_q, st_q = got.render(b, e.sun, W, H, mode=mode)
        ok, bad = ppm_budget_ok(pkg.ppm(W, H, rgb_q), pkg.ppm(W, H, rgb_e), W, H)
        assert ok, f"{bad} pixels beyond +-1 LSB"
        _, _, sh_e, _ = got.records(b, e.sun, W, H, mode=e.full)
        _, _, sh_q, _ = got.records(b, e.sun, W, H, mode=mode)
        darkened = int(np.count_nonzero((sh_e == 0) & (sh_q == 1)))
        assert int(np.count_nonzero((sh_e == 1) & (sh_q == 0))) == 0, "an occluded pixel turned lit"
        assert np.array_equal(sh_e == -1, sh_q == -1)
        assert st_q["rays"] == st_e["rays"] and st_q["hits"] - st_e["hits"] == darkened
        assert darkened <= max(1, int(1e-5 * W * H))


@pytest.mark.parametrize("name,width", WIDE)
def test_stats_scenes(envs, name, width):
    """CERES_SCENE_STATS scenes: the Statistics counters (node pairs, triangle tests) of full and
    primary-only frames, fast and robust, and the per-pixel hit records."""
    e = envs(name)
    pkg = e.pkg
    for arith, fma in ((pkg.ARITH_EXACT, 0), (pkg.ARITH_FMA, pkg.MODE_FMA)):
        got, nat = e.scene(width, arith, "stats"), e.scene(None, arith, "stats")
        W, H = SIZES[1]
        for view in ("cfg", "odd"):
            b = e.views(W, H)[view]
            for mode in (pkg.MODE_FULL, pkg.MODE_FULL | pkg.MODE_ROBUST, pkg.MODE_PRIMARY):
                a, n = got.render(b, e.sun, W, H, mode=mode | fma), nat.render(b, e.sun, W, H, mode=mode | fma)
                _same_frame(a, n, f"{name} {view} mode {mode | fma}")
                assert (a[2]["node_pairs"], a[2]["tri_tests"]) == (n[2]["node_pairs"], n[2]["tri_tests"]), (view, mode | fma)
                assert a[2]["node_pairs"] > 0 or name == "tri1"
            ra, rn = got.records(b, e.sun, W, H, mode=pkg.MODE_FULL | fma), nat.records(b, e.sun, W, H, mode=pkg.MODE_FULL | fma)
            assert np.array_equal(ra[0], rn[0]) and np.array_equal(ra[2], rn[2])
            assert np.array_equal(ra[1].view(np.uint32), rn[1].view(np.uint32))
            assert (ra[3]["node_pairs"], ra[3]["tri_tests"], ra[3]["rays"], ra[3]["hits"]) == \
                   (rn[3]["node_pairs"], rn[3]["tri_tests"], rn[3]["rays"], rn[3]["hits"])
        # the production scene's records go through the same stats kernels
        b = e.views(W, H)["cfg"]
        ra, rn = e.scene(width, arith).records(b, e.sun, W, H, mode=pkg.MODE_FULL | fma), \
            e.scene(None, arith).records(b, e.sun, W, H, mode=pkg.MODE_FULL | fma)
        assert np.array_equal(ra[0], rn[0]) and np.array_equal(ra[2], rn[2]) and np.array_equal(ra[1].view(np.uint32), rn[1].view(np.uint32))


def _raw(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint8)


def _rays_of(name):
    return T.adversarial_rays() if name == "dragon_333x217" else T.proc300_window_rays()


QUERY_CASES = [("dragon_333x217", 3), ("dragon_333x217", 4), ("proc_300", 4)]


@pytest.mark.parametrize("kind", ["prod", "stats"])
@pytest.mark.parametrize("name,width", QUERY_CASES)
def test_trace_on_wider_stacks(envs, name, width, kind):
    """ceres_trace_rays_k<Stk24> and <uint32_t*>: closest hit, occlusion and both, production and stats scenes, fast
    and robust, exact and FMA; every answer byte and counter is the natural-width scene's."""
    e = envs(name)
    pkg = e.pkg
    rays = _rays_of(name)
    for arith, fma in ((pkg.ARITH_EXACT, 0), (pkg.ARITH_FMA, pkg.MODE_FMA)):
        got, nat = e.scene(width, arith, kind), e.scene(None, arith, kind)
        if name == "proc_300":
            assert got.info()["n_pairs"] >= 1 << 16
        for robust in (0, pkg.MODE_ROBUST):
            for closest, occluded in ((True, False), (False, True), (True, True)):
                ha, oa, sa = got.trace(rays, mode=fma | robust, closest=closest, occluded=occluded)
                hn, on, sn = nat.trace(rays, mode=fma | robust, closest=closest, occluded=occluded)
                what = f"{name} {kind} fma={fma} robust={robust} closest={closest} occluded={occluded}"
                if closest:
                    assert np.array_equal(_raw(ha), _raw(hn)), what
                    assert (ha["prim"] >= 0).any()
                if occluded:
                    assert np.array_equal(oa, on), what
                    assert oa.any() and not oa.all()
                for k in ("rays", "hits", "node_pairs", "tri_tests"):
                    assert sa[k] == sn[k], (what, k)


@pytest.mark.parametrize("name,width", QUERY_CASES)
def test_shade_on_wider_stacks(envs, name, width):
    """ceres_shade_rays_k<Stk24> and <uint32_t*>: pixels, RGB8, hits and status of the adversarial rays over the
    dragon and of the windowed camera rays over the 300 x 300 heightfield."""
    e = envs(name)
    pkg = e.pkg
    rays = _rays_of(name)
    for arith, fma in ((pkg.ARITH_EXACT, 0), (pkg.ARITH_FMA, pkg.MODE_FMA)):
        got, nat = e.scene(width, arith), e.scene(None, arith)
        for robust in (0, pkg.MODE_ROBUST):
            a = got.shade(rays, e.sun, mode=fma | robust, pixels=True, rgb8=True, hits=True, status=True)
            n = nat.shade(rays, e.sun, mode=fma | robust, pixels=True, rgb8=True, hits=True, status=True)
            for x, y, what in zip(a[:4], n[:4], ("pixels", "rgb8", "hits", "status")):
                assert np.array_equal(_raw(x), _raw(y)), (name, fma, robust, what)
            assert set(np.unique(a[3])) == {0, 1, 2}, "misses, lit and shadowed rays"
            assert (a[4]["rays"], a[4]["hits"]) == (n[4]["rays"], n[4]["hits"])


def _moved(pkg, mesh, root, shift):
    """The mesh with the half of its triangles right of the middle translated along x."""
    tri = mesh.tri.copy()
    cx = tri[:, 0] + (tri[:, 3] + tri[:, 6]) / 3
    tri[cx > 0.5 * (root[0] + root[1]), 0] += np.float32(shift)
    return pkg.Mesh(tri, mesh.norm)


@pytest.mark.parametrize("how", ["refit", "update"])
@pytest.mark.parametrize("name,width", [("proc_300", 3), ("proc_300", 4), ("proc_101", 4)])
def test_upkeep_keeps_the_width(envs, name, width, how):
    """Half of the mesh moved sideways by 0.3 scene diagonals, then a refit, or an update that rebuilds:
    the frames and batches afterwards are a fresh scene's, the width is the one the scene was made with,
    and the QBVH4 copy is requantised (a stale one loses the moved half's shadows)."""
    e = envs(name)
    pkg = e.pkg
    W, H = SIZES[0]
    diag = C.scene_frame(e.root)[1]
    mesh2 = _moved(pkg, e.mesh, e.root, 0.3 * diag)
    root2 = M.root_box(mesh2.tri)
    b12 = np.stack([C.look(pkg, root2, W, H, dist=2.5), C.look(pkg, root2, W, H, yaw=6.0, dist=3.0),
                    np.asarray(e.cam.basis(W, H), np.float32)])
    qmode = e.full | pkg.MODE_QBVH4
    with forced(width):
        scene = pkg.Scene(e.mesh, e.bvh)
    fresh = pkg.Scene(mesh2, pkg.build_bvh(mesh2, pkg.ARITH_FMA))
    try:
        assert scene.stack_width() == width and fresh.stack_width() == NATURAL[name]
        scene.render(b12[2], e.sun, W, H, mode=qmode)                # quantise the old boxes
        if how == "refit":
            scene.refit(mesh2)
        else:
            assert scene.update(mesh2, 1e-9, arith=pkg.ARITH_FMA)["rebuilt"] == 1
        assert scene.stack_width() == width, "the upkeep changed the width"
        if name == "proc_300":
            assert scene.info()["n_pairs"] >= 1 << 16
        want, got = _call(e, fresh, b12, W, H), _call(e, scene, b12, W, H)
        assert got[2][6] == 0 and got[2][:4] == want[2][:4]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert scene.compact_order() is not None and scene.compact_order()["tpw"] == 4
        assert scene.entry_nodes()["used"] == (width == 2)
        for b in b12:
            _same_frame(scene.render(b, e.sun, W, H, mode=e.full), fresh.render(b, e.sun, W, H, mode=e.full), how)
        b = b12[2]
        _, rgb_e, st_e = scene.render(b, e.sun, W, H, mode=e.full)
        _, rgb_q, st_q = scene.render(b, e.sun, W, H, mode=qmode)
        ok, bad = ppm_budget_ok(pkg.ppm(W, H, rgb_q), pkg.ppm(W, H, rgb_e), W, H)
        assert ok, f"{bad} pixels beyond +-1 LSB: the QBVH4 copy was not requantised"
        assert st_q["rays"] == st_e["rays"] and 0 <= st_q["hits"] - st_e["hits"] <= max(1, int(1e-5 * W * H))
        _, _, sh_e, _ = scene.records(b, e.sun, W, H, mode=e.full)
        _, _, sh_q, _ = scene.records(b, e.sun, W, H, mode=qmode)
        assert int(np.count_nonzero((sh_e == 1) & (sh_q == 0))) == 0, "an occluded pixel turned lit"
    finally:
        scene.close()
        fresh.close()


@pytest.mark.parametrize("name,width", [("proc_101", 4), ("proc_300", 4), ("tri1", 3)])
def test_device_made_scenes_read_the_hook_too(envs, name, width):
    """ceres_scene_create_device (GPU-built BVH, device relayout): the width is read there as well; a solo
    frame and a compacting batch equal the host-made natural-width scene's."""
    import torch
    e = envs(name)
    pkg = e.pkg
    n = len(e.mesh)
    d_tri = torch.from_numpy(e.mesh.tri.reshape(-1).copy()).to("cuda:0")
    d_norm = torch.from_numpy(e.mesh.norm.reshape(-1).copy()).to("cuda:0")
    d_nodes = torch.empty((2 * n - 1) * 8 if n > 1 else 8, dtype=torch.int32, device="cuda:0")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    m = pkg.build_bvh_device(d_tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), stream, pkg.ARITH_FMA)
    with forced(width):
        sc = pkg.Scene.from_device(d_tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stream=stream)
    try:
        assert sc.stack_width() == width
        W, H = SIZES[1]
        v = e.views(W, H)
        _same_frame(sc.render(v["cfg"], e.sun, W, H, mode=e.full), e.scene().render(v["cfg"], e.sun, W, H, mode=e.full), name)
        _parity(e, sc, np.stack([v["odd"], v["gone"], v["cfg"]]), W, H)
        _check_batch_path(e, sc, width)
    finally:
        sc.close()


@pytest.fixture(scope="module")
def count_build(pkg):
    """variants/libceres_hip_count.so (the stack guard compiled in) behind a second copy of the package."""
    pkgdir = os.path.dirname(pkg.__file__)
    path = os.path.join(pkgdir, "variants", "libceres_hip_count.so")
    assert os.path.exists(path), "the diagnostic build is part of build() (make all)"
    spec = importlib.util.spec_from_file_location("ceres_count_build_widths", os.path.join(pkgdir, "__init__.py"),
                                                  submodule_search_locations=[pkgdir])
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    cb.LIB_PATH = path
    cb.lib()
    return cb


@pytest.mark.parametrize("width", [3, 4])
def test_counting_build_guards_stay_clear(envs, count_build, width):
    """The guarded walks of the diagnostic build keep 0xffffff (Stk24) and 0xffffffff (uint32_t*) in slot
    stack_entries (render_hip.hip pins the two values at compile time): a solo frame and a compacting
    batch of proc_300 leave the error word 0 and render the product's bytes."""
    e = envs("proc_300")
    sc = e.scene(width, mod=count_build)
    assert sc.info()["n_pairs"] >= 1 << 16
    W, H = SIZES[1]
    v = e.views(W, H)
    _same_frame(sc.render(v["cfg"], e.sun, W, H, mode=e.full), e.scene().render(v["cfg"], e.sun, W, H, mode=e.full), "solo")
    _parity(e, sc, np.stack([v["odd"], v["gone"], v["cfg"]]), W, H)
    _check_batch_path(e, sc, width)


@pytest.mark.parametrize("prefix,records,width", [(PREFIX_LAST_16, 65535, 2), (PREFIX_FIRST_24, 65536, 3)])
def test_the_16_24_bit_threshold(pkg, envs, prefix, records, width):
    """The last 16-bit scene and the first 24-bit one.  The first `prefix` triangles of proc_mesh(260)
    (134,162 triangles; a prefix is an ordinary triangle soup) under build_bvh, both ARITH_FMA: a host
    search over the prefixes 120,800 .. 121,799 (ceres_entry_relayout's pair count, which is not
    monotonic in the length) found 65,535 pairs at 121,765 and 121,766 and 65,536 pairs at 121,767 and
    121,768 -- both values are met exactly.  A BVH4 record stands for an inner BVH2 node, so there are
    no more of them than pairs and the pair count decides.  With 65,535 records the top index is 65,534
    and the 16-bit guard value 0xffff stays free; with 65,536 it would be a node index.
    One 136x72 solo frame and one 3-frame batch of each equal CpuScene.render of the same mesh and
    BVH bit for bit; the error word is 0."""
    full = pkg.proc_mesh(260, pkg.ARITH_FMA)
    mesh = pkg.Mesh(full.tri[:prefix].copy(), full.norm[:prefix].copy())
    bvh = pkg.build_bvh(mesh, pkg.ARITH_FMA)
    assert len(pkg.entry_relayout(mesh, bvh)[0]) == records
    e = envs("proc_101")                                             # its sun and helpers; the scenes are this test's
    gpu, cpu = pkg.Scene(mesh, bvh), pkg.CpuScene(mesh, bvh)
    try:
        assert gpu.info()["n_pairs"] == records and gpu.stack_width() == width
        nodes4 = gpu.read_boxes()[1]
        assert nodes4 is not None and len(nodes4) <= records
        W, H = SIZES[0]
        root = M.root_box(mesh.tri)
        b12 = np.stack([C.look(pkg, root, W, H), C.look(pkg, root, W, H, yaw=9.0, pitch=-4.0, dist=2.5),
                        C.look(pkg, root, W, H, yaw=60.0)])
        want = [cpu.render(b, e.sun, W, H, mode=e.full) for b in b12]
        assert want[0][2]["hits"] > 0 and want[2][2]["rays"] == W * H
        _same_frame(gpu.render(b12[0], e.sun, W, H, mode=e.full), want[0], "solo", keys=("rays", "hits"))
        px, rgb, c = _call(e, gpu, b12, W, H)
        assert c[6] == 0
        assert gpu.compact_order() is not None and gpu.entry_nodes()["used"] == (width == 2)
        for f, (wp, wr, ws) in enumerate(want):
            assert np.array_equal(px[f], wp.view(np.uint8)) and np.array_equal(rgb[f], wr), f"frame {f}"
        assert c[0] == sum(w[2]["rays"] for w in want) and c[1] == sum(w[2]["hits"] for w in want)
    finally:
        gpu.close()
        cpu.close()
