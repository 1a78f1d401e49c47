"""Indexed ray queries and the coherent ray order on the GPU (ceres_*_indexed_device, ceres_ray_order_device,
ceres_trace_rays_coherent; Scene.*_device(d_index=...), Scene.ray_order_device, Scene.trace(coherent=True),
`./render --rays --coherent`).

Lane i of an indexed launch takes ray index[i] and writes that ray's own output slots.  Pinned here: the GPU
order to the CPU order (itself pinned to a numpy model by test_rayorder_cpu.py); the identity list to the plain
call, byte for byte, all eight calls; the reference's stored answers through a random permutation and through
the coherent order; subsets with invalid and duplicate entries against pre-filled output buffers; the lists flow
on survivors; the three stack widths; the refusals; the coherent host call and the CLI; the render calls."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import allhits64_common as a64
import allhits_common as ac
import rayorder_common as ro
import trace64_common as t64
import trace_common as tc

pytestmark = pytest.mark.gpu

FILL = 0x5a
PAD = 256                                                             # guard bytes on either side (keeps the alignment)
K = 4                                                                 # max_hits of the all-hits rows
LENGTHS = (1, 63, 64, 65, 4097)
FAMILIES = ("trace", "all", "lists", "shade")


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return pkg


@contextlib.contextmanager
def env(**kv):
    """Environment variables while a scene is created (the hooks are read then and only then)."""
    old = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Buf:
    """`nbytes` device bytes between two guard regions, everything pre-filled with FILL."""

    def __init__(self, nbytes):
        import torch
        self.n = int(nbytes)
        self.t = torch.full((self.n + 2 * PAD,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + PAD

    def body(self):
        return self.t[PAD:PAD + self.n].cpu().numpy()

    def guards_intact(self):
        a = self.t.cpu().numpy()
        return bool((a[:PAD] == FILL).all() and (a[PAD + self.n:] == FILL).all())


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def scene_of(gpu, cache, key, make, **kw):
    if key not in cache:
        cache[key] = gpu.Scene(*make(), **kw)
    return cache[key]


@pytest.fixture(scope="module")
def scenes(gpu):
    cache = {}

    class Get:
        def __call__(self, name, arith=0, stats=False):
            if name.endswith("64"):
                make = (lambda: a64.set_scene(name, "ref" if arith else "exact")) if name == a64.DUPLEAF64 else \
                       (lambda: t64.ray_set_scene(name, "ref" if arith else "exact"))
                key = (name, arith, stats)
            else:
                make = lambda: ac.all_set_scene(name, arith)
                key = (ac.scene_key(name), arith, stats)
            return scene_of(gpu, cache, key, make, stats=stats)

        def cpu(self, name):
            key = (name, "cpu")
            if key not in cache:
                cache[key] = gpu.CpuScene(*ro.set_scene(name))
            return cache[key]

        def quad_view(self, f64):
            """(scene, rays, sun) of the quad_65x49 view's camera rays."""
            cfg, mesh, bvh, basis, sun = tc.fixture("quad_65x49_robust", 0)[:5]
            if not f64:
                return scene_of(gpu, cache, ("quadview", 0), lambda: (mesh, bvh)), gpu.camera_rays(basis, cfg["W"], cfg["H"]), sun
            sc = scene_of(gpu, cache, ("quadview", 1), lambda: gpu.prepare(cfg, f64=True, arith=0)[:2])
            return sc, gpu.camera_rays64(np.asarray(basis, np.float64), cfg["W"], cfg["H"]), np.asarray(sun, np.float64)

    yield Get()
    for s in cache.values():
        s.close()


def set_rays(name):
    return a64.set_rays(name) if name == a64.DUPLEAF64 else (ro.set_rays(name) if name.endswith("64") or name in ro.FLOAT_SETS
                                                            else np.ascontiguousarray(ac.load_all_fixture(name)["rays"]))


def offsets_for(gpu, sc, d_rays, n, mode):
    """The plain count-only query and the scan: (offsets u64 [n + 1] on the host, the device tensor)."""
    import torch
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    nb = gpu.hit_offsets_scratch_bytes(n)
    scr = torch.zeros(nb // 8 + 1, dtype=torch.int64, device="cuda")
    sc.trace_all_device(d_rays.data_ptr(), n, mode=mode, d_counts=cnt.data_ptr())
    sc.hit_offsets_device(cnt.data_ptr(), n, off.data_ptr(), scr.data_ptr(), nb)
    torch.cuda.synchronize()
    return off.cpu().numpy().view(np.uint64), off


def run(gpu, sc, fam, d_rays, n, mode, index=None, sun=None, off=None, total=0, expect=None):
    """One device call of a family into pre-filled, guarded buffers; index: None for the plain call, else a
    uint32 array.  Returns ({output: bytes as uint8 array}, counters u64 [8]).  expect: the status the call
    must be refused with (then the outputs are returned untouched)."""
    import torch
    hb, pb = (32, 24) if sc.f64 else (16, 12)
    sizes = {"trace": {"hits": n * hb, "occ": n}, "all": {"counts": 4 * n, "rows": n * K * hb},
             "shade": {"px": n * pb, "rgb": 3 * n, "hits": n * hb, "status": n}, "lists": {"hits": total * hb}}[fam]
    b = {k: Buf(v) for k, v in sizes.items()}
    ctr = Buf(64)
    ix = {}
    if isinstance(index, dict):                                       # raw arguments (refusal tests)
        ix = index
    elif index is not None:
        d_idx = to_device(index)
        ix = dict(d_index=d_idx.data_ptr() if len(index) else 0, n_index=len(index))
    call = {"trace": lambda: sc.trace_device(d_rays.data_ptr(), n, mode=mode, d_hits16=b["hits"].ptr(), d_occluded=b["occ"].ptr(),
                                             d_counters=ctr.ptr(), **ix),
            "all": lambda: sc.trace_all_device(d_rays.data_ptr(), n, max_hits=K, mode=mode, d_counts=b["counts"].ptr(),
                                               d_hits16=b["rows"].ptr(), d_counters=ctr.ptr(), **ix),
            "shade": lambda: sc.shade_device(d_rays.data_ptr(), n, sun, mode=mode, d_pixels=b["px"].ptr(), d_rgb8=b["rgb"].ptr(),
                                             d_hits16=b["hits"].ptr(), d_status=b["status"].ptr(), d_counters=ctr.ptr(), **ix),
            "lists": lambda: sc.trace_lists_device(d_rays.data_ptr(), n, off.data_ptr(), b["hits"].ptr(), total, mode=mode,
                                                   d_counters=ctr.ptr(), **ix)}[fam]
    if expect is not None:
        with pytest.raises(gpu.CeresError) as e:
            call()
        assert ("ceres error %d:" % expect) in str(e.value), str(e.value)
    else:
        call()
    torch.cuda.synchronize()
    assert ctr.guards_intact() and all(x.guards_intact() for x in b.values()), (fam, "a guard region was written")
    return {k: x.body() for k, x in b.items()}, ctr.body().view(np.uint64)


def untouched(out, ctr=None):
    return all((a == FILL).all() for a in out.values()) and (ctr is None or (ctr.view(np.uint8) == FILL).all())


def family_case(gpu, scenes, fam, f64):
    """(scene, rays, sun) of the family's first set."""
    if fam == "shade":
        return scenes.quad_view(f64)
    name = {"trace": "dragon_adversarial", "all": "quad_tiny", "lists": "quad_tiny"}[fam] + ("64" if f64 else "")
    return scenes(name), set_rays(name), None


def modes_of(gpu, f64):
    return [0, gpu.MODE_FMA] if f64 else [0, gpu.MODE_FMA, gpu.MODE_ROBUST, gpu.MODE_FMA | gpu.MODE_ROBUST]


# ---------------------------------------------------------------- the order
def device_order(gpu, sc, rays, n, stream=None, scratch_pad=PAD):
    """ray_order_device on the first n rays; d_order and the scratch between guards.  Returns a closure that
    synchronises, checks the guards and gives the order."""
    import torch
    d_rays = to_device(rays[:n])
    order, nb = Buf(4 * n), gpu.ray_order_scratch_bytes(n)
    scr = Buf(nb)
    sc.ray_order_device(d_rays.data_ptr(), n, order.ptr(), scr.ptr(), nb, stream=stream.cuda_stream if stream else 0)

    def finish():
        (stream.synchronize() if stream else torch.cuda.synchronize())
        assert order.guards_intact() and scr.guards_intact(), "a guard region around d_order or the scratch was written"
        del d_rays_keep[:]
        return order.body().view(np.uint32)

    d_rays_keep = [d_rays]
    return finish


@pytest.mark.parametrize("name", ro.FLOAT_SETS + ro.DOUBLE_SETS)
def test_gpu_order_equals_the_cpu_order(gpu, scenes, name):
    rays = ro.set_rays(name)
    for n in (1, 63, 64, 65, len(rays)):
        got = device_order(gpu, scenes(name), rays, n)()
        exp = scenes.cpu(name).ray_order(rays[:n])
        assert np.array_equal(got, exp), (name, n, "first differing place", np.flatnonzero(got != exp)[:4])


def test_gpu_order_on_two_streams(gpu, scenes):
    import torch
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, b = ro.set_rays("dragon_adversarial"), ro.set_rays("lattice_ties")
    with torch.cuda.stream(s0):
        fa = device_order(gpu, scenes("dragon_adversarial"), a, len(a), stream=s0)
    with torch.cuda.stream(s1):
        fb = device_order(gpu, scenes("lattice_ties"), b, len(b), stream=s1)
    assert np.array_equal(fa(), scenes.cpu("dragon_adversarial").ray_order(a))
    assert np.array_equal(fb(), scenes.cpu("lattice_ties").ray_order(b))


# ---------------------------------------------------------------- identity list
@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_identity_list_equals_the_plain_call(gpu, scenes, fam, f64):
    """index = arange(n): every output byte and all 8 counter words are the plain call's."""
    cases = [family_case(gpu, scenes, fam, f64)]
    if fam in ("all", "lists"):
        name = a64.DUPLEAF64 if f64 else ac.DUPLEAF
        cases.append((scenes(name), set_rays(name), None))
    for sc, rays, sun in cases:
        n, d_rays = len(rays), to_device(rays)
        for mode in modes_of(gpu, f64):
            kw = {}
            if fam == "lists":
                offs, d_off = offsets_for(gpu, sc, d_rays, n, mode)
                kw = dict(off=d_off, total=int(offs[n]))
            plain, pc = run(gpu, sc, fam, d_rays, n, mode, sun=sun, **kw)
            got, gc = run(gpu, sc, fam, d_rays, n, mode, index=np.arange(n, dtype=np.uint32), sun=sun, **kw)
            for k in plain:
                assert np.array_equal(got[k], plain[k]), (fam, f64, mode, k, np.flatnonzero(got[k] != plain[k])[:4])
            assert np.array_equal(gc, pc), (fam, f64, mode, gc, pc)
            assert not untouched(plain)


# ---------------------------------------------------------------- the reference through a permutation
def through_lists(gpu, sc, rays, mode, exp_hits, exp_occ, where):
    """trace_device(d_index=...) over a fixed random permutation, then over the coherent order: the stored
    reference answers for every ray, no tolerance."""
    n, d_rays = len(rays), to_device(rays)
    order = device_order(gpu, sc, rays, n)()
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    for label, index in (("permutation", ro.random_permutation(n)), ("coherent order", order)):
        out, c = run(gpu, sc, "trace", d_rays, n, mode, index=index)
        assert out["hits"].tobytes() == exp_hits.tobytes(), (where, label)
        assert np.array_equal(out["occ"], exp_occ), (where, label)
        assert c[0] == n and c[2] == n and c[1] == int((exp_hits["prim"] >= 0).sum()) and c[6] == 0, (where, label, c)


@pytest.mark.parametrize("variant", tc.RAY_VARIANTS)
@pytest.mark.parametrize("name", tc.RAY_SETS)
def test_reference_answers_through_index_lists(gpu, scenes, name, variant):
    mode, arith = tc.variant_mode(gpu, variant)
    fx = tc.load_ray_fixture(name)
    ref = fx[variant]
    through_lists(gpu, scenes(name, arith), np.ascontiguousarray(fx["rays"]), mode, tc.reference_hits(gpu, ref),
                  ref["occluded"].astype(np.uint8), (name, variant))


@pytest.mark.parametrize("variant", t64.RAY_VARIANTS64)
@pytest.mark.parametrize("name", t64.RAY_SETS64)
def test_reference_answers_through_index_lists_f64(gpu, scenes, name, variant):
    mode, build = t64.variant_mode(gpu, variant)
    fx = t64.load_ray_fixture64(name)
    ref = fx[variant]
    through_lists(gpu, scenes(name, 1 if build == "ref" else 0), np.ascontiguousarray(fx["rays"]), mode,
                  t64.reference_hits(gpu, ref), ref["occluded"].astype(np.uint8), (name, variant))


# ---------------------------------------------------------------- subsets and bad entries
def record_sizes(fam, f64):
    hb, pb = (32, 24) if f64 else (16, 12)
    return {"trace": {"hits": hb, "occ": 1}, "all": {"counts": 4, "rows": K * hb},
            "shade": {"px": pb, "rgb": 3, "hits": hb, "status": 1}}[fam]


def check_subset(gpu, sc, fam, f64, d_rays, n, sun, plain, index, mode=0, kw=None, offs=None):
    out, c = run(gpu, sc, fam, d_rays, n, mode, index=index, sun=sun, **(kw or {}))
    listed = np.zeros(n, bool)
    listed[ro.valid_rays(index, n)] = True
    where = (fam, f64, len(index))
    if fam == "lists":                                                # the listed rays' segments; the rest is unspecified
        hb = 32 if f64 else 16
        got, exp = out["hits"].reshape(-1, hb), plain["hits"].reshape(-1, hb)
        for r in np.flatnonzero(listed):
            assert np.array_equal(got[int(offs[r]):int(offs[r + 1])], exp[int(offs[r]):int(offs[r + 1])]), (where, "ray", r)
    else:
        for k, rs in record_sizes(fam, f64).items():
            got, exp = out[k].reshape(n, rs), plain[k].reshape(n, rs)
            assert np.array_equal(got[listed], exp[listed]), (where, k, "a listed ray differs from the plain call")
            assert (got[~listed] == FILL).all(), (where, k, "an unlisted ray's output was written")
    assert c[2] == len(index) and (fam == "shade" or c[0] == len(index)), (where, c)
    assert c[6] == 0
    return out, c


@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_subsets_and_bad_entries(gpu, scenes, fam, f64):
    """Every third ray plus the entries n_rays, n_rays + 1 and 0xffffffff plus one duplicate, at the lengths
    1, 63, 64, 65 and 4,097; a whole wavefront of invalid entries; the empty list."""
    sc, rays, sun = family_case(gpu, scenes, fam, f64)
    n, d_rays = len(rays), to_device(rays)
    kw, offs = {}, None
    if fam == "lists":
        offs, d_off = offsets_for(gpu, sc, d_rays, n, 0)
        kw = dict(off=d_off, total=int(offs[n]))
    plain, _ = run(gpu, sc, fam, d_rays, n, 0, sun=sun, **kw)
    for length in LENGTHS:
        index = ro.subset_with_bad_entries(n, length)
        if fam == "lists":                                            # distinct entries: the duplicates become invalid ones
            _, first = np.unique(index, return_index=True)
            dup = np.ones(length, bool)
            dup[first] = False
            index = np.where(dup, np.uint32(0xfffffffe), index).astype(np.uint32)
        elif length >= 8:
            v = index[index < n]
            assert len(v) > len(np.unique(v)) and (index >= n).sum() == 3     # the list's own conditions
        check_subset(gpu, sc, fam, f64, d_rays, n, sun, plain, index, kw=kw, offs=offs)
    dead = np.asarray([n, n + 1, 0xffffffff] * 21 + [n], np.uint32)   # 64 invalid entries: a wavefront that does nothing
    out, c = run(gpu, sc, fam, d_rays, n, 0, index=dead, sun=sun, **kw)
    assert untouched(out) and c[2] == 64 and c[1] == 0 and c[3] == 0, (fam, f64, c)
    out, c = run(gpu, sc, fam, d_rays, n, 0, index=np.zeros(0, np.uint32), sun=sun, **kw)
    assert untouched(out, c), (fam, f64, "n_index = 0 is a no-op")


# ---------------------------------------------------------------- the lists flow on survivors
@pytest.mark.parametrize("name", ["tri1_tiny", "lattice_ties", "tri1_tiny64", "lattice_ties64"])
def test_lists_flow_on_survivors(gpu, scenes, name):
    """Count-only indexed over a subset, the scan, the indexed fill over the same subset: the listed rays'
    segments are the plain flow's."""
    import torch
    sc, rays = scenes(name), set_rays(name)
    f64, n, d_rays = name.endswith("64"), len(rays), to_device(rays)
    hb = 32 if f64 else 16
    offs, d_off = offsets_for(gpu, sc, d_rays, n, 0)
    plain, _ = run(gpu, sc, "lists", d_rays, n, 0, off=d_off, total=int(offs[n]))
    index = ro.every_third(n)
    d_idx = to_device(index)
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")            # unlisted rays: no hits
    off2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    nb = gpu.hit_offsets_scratch_bytes(n)
    scr = torch.zeros(nb // 8 + 1, dtype=torch.int64, device="cuda")
    sc.trace_all_device(d_rays.data_ptr(), n, d_counts=cnt.data_ptr(), d_index=d_idx.data_ptr(), n_index=len(index))
    sc.hit_offsets_device(cnt.data_ptr(), n, off2.data_ptr(), scr.data_ptr(), nb)
    torch.cuda.synchronize()
    offs2 = off2.cpu().numpy().view(np.uint64)
    counts = np.diff(offs.astype(np.int64))
    assert np.array_equal(np.diff(offs2.astype(np.int64))[index], counts[index]) and int(offs2[n]) == int(counts[index].sum())
    assert int(offs2[n]) > 0
    out, c = run(gpu, sc, "lists", d_rays, n, 0, index=index, off=off2, total=int(offs2[n]))
    got, exp = out["hits"].reshape(-1, hb), plain["hits"].reshape(-1, hb)
    for r in index:
        assert np.array_equal(got[int(offs2[r]):int(offs2[r + 1])], exp[int(offs[r]):int(offs[r + 1])]), (name, "ray", r)
    assert c[0] == len(index) and c[3] == int(offs2[n]) and c[6] == 0 and c[7] == 0, (name, c)


# ---------------------------------------------------------------- stack widths
@pytest.mark.parametrize("name", ["quad_tiny", "lattice_ties"])
def test_indexed_answers_do_not_depend_on_the_stack_width(gpu, scenes, name):
    """Scenes created under CERES_DEBUG_STACK_WIDTH=3 and =4 (the natural width of these is 2): the same
    indexed answers, all four families' float kernels."""
    rays = set_rays(name)
    n, d_rays = len(rays), to_device(rays)
    index = ro.subset_with_bad_entries(n, 65)
    sun = np.asarray([-3, 9, 2.5], np.float32)
    offs, d_off = offsets_for(gpu, scenes(name), d_rays, n, 0)
    lists_index = np.unique(index)
    base = {}
    for width in (None, 3, 4):
        if width is None:
            sc = scenes(name)
        else:
            with env(CERES_DEBUG_STACK_WIDTH=width):
                sc = gpu.Scene(*ac.all_set_scene(name, 0))
        try:
            assert width is None or sc.stack_width() == width
            for fam in FAMILIES:
                kw = dict(off=d_off, total=int(offs[n])) if fam == "lists" else {}
                out, c = run(gpu, sc, fam, d_rays, n, 0, index=lists_index if fam == "lists" else index, sun=sun, **kw)
                if width is None:
                    base[fam] = (out, c)
                else:
                    for k in out:
                        assert np.array_equal(out[k], base[fam][0][k]), (name, width, fam, k)
                    assert np.array_equal(c, base[fam][1]), (name, width, fam)
        finally:
            if width is not None:
                sc.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
def test_refusals_leave_the_outputs_alone(gpu, scenes, f64):
    import torch
    name = "quad_tiny64" if f64 else "quad_tiny"
    other = "quad_tiny" if f64 else "quad_tiny64"
    rays = set_rays(name)
    n, d_rays = len(rays), to_device(rays)
    sun = np.asarray([-3, 9, 2.5], np.float64 if f64 else np.float32)
    d_idx = to_device(np.arange(n + 1, dtype=np.uint32))
    offs, d_off = offsets_for(gpu, scenes(name), d_rays, n, 0)
    stats_scene = scenes(name, 0, True)
    for fam in FAMILIES:
        kw = dict(off=d_off, total=int(offs[n])) if fam == "lists" else {}
        bad = [(scenes(name), dict(d_index=d_idx.data_ptr() + 2, n_index=n), -1),      # misaligned
               (scenes(name), dict(d_index=0, n_index=n), -1),                           # NULL with n_index > 0
               (scenes(name), dict(d_index=d_idx.data_ptr(), n_index=1 << 31), -6),
               (stats_scene, dict(d_index=d_idx.data_ptr(), n_index=n), -6),
               (scenes(other), dict(d_index=d_idx.data_ptr(), n_index=n), -6)]           # the other precision's scene
        for sc, ix, status in bad:
            wrong = sc.f64 != f64                                     # the methods dispatch on Scene.f64: make them call
            sc.f64 = f64                                              # this precision's C function with the other's scene
            try:
                out, c = run(gpu, sc, fam, d_rays, n, 0, index=ix, sun=sun, expect=status, **kw)
            finally:
                sc.f64 = f64 != wrong
            assert untouched(out, c), (fam, f64, ix, "a refused call wrote")
    # the order: the other precision's scene, a small and a misaligned scratch
    nb = gpu.ray_order_scratch_bytes(n)
    order, scr = Buf(4 * n), Buf(nb)
    for sc, args in ((scenes(other), (order.ptr(), scr.ptr(), nb)), (scenes(name), (order.ptr(), scr.ptr(), nb - 1)),
                     (scenes(name), (order.ptr(), scr.ptr() + 4, nb)), (scenes(name), (order.ptr(), 0, nb)),
                     (scenes(name), (0, scr.ptr(), nb))):
        wrong = sc.f64 != f64
        sc.f64 = f64
        try:
            with pytest.raises(gpu.CeresError) as e:
                sc.ray_order_device(d_rays.data_ptr(), n, *args)
        finally:
            sc.f64 = f64 != wrong
        assert ("ceres error %d:" % (-6 if wrong else -1)) in str(e.value)
    torch.cuda.synchronize()
    assert (order.t.cpu().numpy() == FILL).all() and (scr.t.cpu().numpy() == FILL).all()


# ---------------------------------------------------------------- the coherent host call
@pytest.mark.parametrize("name", ["dragon_adversarial", "dragon_adversarial64"])
def test_coherent_host_call_returns_the_plain_calls_bytes(gpu, scenes, name):
    rays, sc = set_rays(name), scenes(name)
    for mode in modes_of(gpu, name.endswith("64")):
        h, o, st = sc.trace(rays, mode=mode, closest=True, occluded=True)
        hc, oc, stc = sc.trace(rays, mode=mode, closest=True, occluded=True, coherent=True)
        assert h.tobytes() == hc.tobytes() and np.array_equal(o, oc), (name, mode)
        assert (st["rays"], st["hits"]) == (stc["rays"], stc["hits"]) and stc["ms"] > 0
    with pytest.raises(gpu.CeresError) as e:
        scenes(name, 0, True).trace(rays, coherent=True)
    assert "ceres error -6:" in str(e.value)
    assert sc.trace(rays[:0], coherent=True)[2]["rays"] == 0


@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_cli_coherent_writes_the_same_files(gpu, tmp_path, double):
    """./render --rays ... --coherent: the files of the run without the flag, byte for byte."""
    rays = ro.set_rays("lattice_ties64" if double else "lattice_ties")
    rf = tmp_path / "rays.bin"
    rf.write_bytes(rays.tobytes())
    exe = os.path.join(os.path.dirname(gpu.__file__), "render")
    files = {}
    for tag, extra in (("plain", []), ("coherent", ["--coherent"])):
        hf, of = tmp_path / (tag + ".hits"), tmp_path / (tag + ".occ")
        cmd = [exe, tc.LATTICE_OBJ, "--exact", "--rays", str(rf), "--hits-out", str(hf), "--occluded-out", str(of)] + extra
        subprocess.run(cmd + (["--double"] if double else []), check=True, capture_output=True, timeout=120)
        files[tag] = (hf.read_bytes(), of.read_bytes())
    assert files["plain"] == files["coherent"] and len(files["plain"][0]) == len(rays) * (32 if double else 16)
    bad = subprocess.run([exe, tc.LATTICE_OBJ, "--coherent"], capture_output=True, timeout=120)
    assert bad.returncode == 2


# ---------------------------------------------------------------- the render calls
def test_render_calls_are_unchanged_by_indexed_calls(gpu, scenes):
    """One frame of quad_65x49 before and after an indexed call and an order call on the same scene."""
    cfg, mesh, bvh, basis, sun = tc.fixture("quad_65x49_robust", 0)[:5]
    sc, rays, _ = scenes.quad_view(False)
    mode = tc.mode_of(gpu, "quad_65x49_robust")
    before = sc.render(basis, sun, cfg["W"], cfg["H"], mode)
    n, d_rays = len(rays), to_device(rays)
    order = device_order(gpu, sc, rays, n)()
    run(gpu, sc, "shade", d_rays, n, 0, index=order, sun=sun)
    run(gpu, sc, "trace", d_rays, n, 0, index=order)
    after = sc.render(basis, sun, cfg["W"], cfg["H"], mode)
    assert np.asarray(before[0]).tobytes() == np.asarray(after[0]).tobytes()
    assert np.asarray(before[1]).tobytes() == np.asarray(after[1]).tobytes()
    assert (before[2]["rays"], before[2]["hits"]) == (after[2]["rays"], after[2]["hits"])
