"""The refusals of the ray-query entry points: status AND ceres_last_error() text, call by call.

Every argument error that is refused on the host, before any launch, for the 24 query entry points (closest/
occlusion, all-hits, complete hit lists and shaded rays; float and double; host-array, device and indexed device
call), the two ceres_ray_order*_device calls, the two coherent calls and ceres_hit_offsets_device.  Each call's
(status, message) is compared with tests/golden/refusals/query_refusals.json (a folder of its own: the
JSON files directly under tests/golden/ are the render configs), recorded once from the library before the
entry points came to share one host layer:

    python tests/test_gpu_query_refusals.py --record        (CERES_LIB=<that build's libceres_hip.so>)

Nothing is launched: every pointer that is not the subject of a case is a real buffer of the right size, and a
call that is not refused where it must be fails the test before its message is looked at."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals", "query_refusals.json")
N = 8                                                                 # rays of every call
K = 4                                                                 # max_hits where a hit buffer is given
CAP = 64                                                              # capacity of the lists calls' hit buffer
MAX_HITS = 32                                                         # CERES_MAX_HITS
FAMILIES = ("trace_rays", "trace_rays_all", "trace_rays_lists", "shade_rays")
FORMS = ("", "_device", "_indexed_device")
vp, sz, ci, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64

# argument names of each entry point, in the C order (ceres_render.h); the same for float and double
ARGS = {
    ("trace_rays", ""): "scene rays n mode hits occluded stats",
    ("trace_rays", "_device"): "scene rays n mode hits occluded counters stream",
    ("trace_rays", "_indexed_device"): "scene rays n index n_index mode hits occluded counters stream",
    ("trace_rays_all", ""): "scene rays n mode max_hits counts hits stats",
    ("trace_rays_all", "_device"): "scene rays n mode max_hits counts hits counters stream",
    ("trace_rays_all", "_indexed_device"): "scene rays n index n_index mode max_hits counts hits counters stream",
    ("trace_rays_lists", ""): "scene rays n mode offsets hits capacity total stats",
    ("trace_rays_lists", "_device"): "scene rays n mode offsets hits capacity counters stream",
    ("trace_rays_lists", "_indexed_device"): "scene rays n index n_index mode offsets hits capacity counters stream",
    ("shade_rays", ""): "scene rays n sun mode pixels rgb8 hits status stats",
    ("shade_rays", "_device"): "scene rays n sun mode pixels rgb8 hits status counters stream",
    ("shade_rays", "_indexed_device"): "scene rays n index n_index sun mode pixels rgb8 hits status counters stream",
    "ray_order": "scene rays n order scratch scratch_bytes stream",
    "coherent": "scene rays n mode hits occluded stats",
    "hit_offsets": "scene counts n offsets scratch scratch_bytes stream",
}
CTYPE = {"n": sz, "n_index": sz, "scratch_bytes": sz, "mode": ci, "max_hits": u32, "capacity": u64}   # every other one: void*


def entry_name(fam, form, f64):
    """ceres_trace_rays_all + _f64 + _indexed_device, as ceres_render.h spells them."""
    return "ceres_" + fam + ("_f64" if f64 else "") + form


def open_library(pkg):
    """A handle of this module's own on the package's library: untyped pointers throughout."""
    pkg.lib()                                                         # loaded the package's way first (one HIP runtime with torch)
    L = ctypes.CDLL(pkg.LIB_PATH)
    L.ceres_last_error.restype = ctypes.c_char_p
    L.ceres_ray_order_scratch_bytes.restype = L.ceres_hit_offsets_scratch_bytes.restype = sz
    L.ceres_ray_order_scratch_bytes.argtypes = L.ceres_hit_offsets_scratch_bytes.argtypes = [sz]
    return L


def call(L, name, names, values):
    """(status, message) of one call; the message of a successful call is not looked at."""
    fn = getattr(L, name)
    fn.restype = ci
    fn.argtypes = [CTYPE.get(a, vp) for a in names]
    status = fn(*[values[a] for a in names])
    return [int(status), L.ceres_last_error().decode() if status else ""]


def entry_points():
    """(key, C name, argument names, f64) of all 29."""
    for f64 in (False, True):
        for fam in FAMILIES:
            for form in FORMS:
                yield (fam, form), entry_name(fam, form, f64), ARGS[(fam, form)].split(), f64
        sfx = "_f64" if f64 else ""
        yield "ray_order", "ceres_ray_order" + sfx + "_device", ARGS["ray_order"].split(), f64
        yield "coherent", "ceres_trace_rays_coherent" + sfx, ARGS["coherent"].split(), f64
    yield "hit_offsets", "ceres_hit_offsets_device", ARGS["hit_offsets"].split(), False


def cases_of(key, f64, gpu_args):
    """[(case, {argument: value})]: the overrides of one refused (or empty) call of this entry point; gpu_args
    gives the other scenes and the sizes."""
    A, out = gpu_args, []
    fam, form = key if isinstance(key, tuple) else (key, "")
    query, device = isinstance(key, tuple), isinstance(key, tuple) and form != ""
    bad_bit = 1 << 20                                                 # outside CERES_MODE_FMA | CERES_MODE_ROBUST
    if key != "hit_offsets":
        out.append(("other_precision", {"scene": A["other_scene"]}))
    if query or key == "coherent":
        out.append(("bad_mode", {"mode": bad_bit}))
        if f64:
            out.append(("robust_on_double", {"mode": A["ROBUST"]}))
    if key == "coherent":
        out.append(("stats_scene", {"scene": A["stats_scene"]}))
    if fam == "trace_rays" or key == "coherent":
        out.append(("no_output", {"hits": 0, "occluded": 0}))
    if fam == "trace_rays_all":
        out += [("no_output", {"counts": 0, "hits": 0}), ("max_hits_0", {"max_hits": 0}), ("max_hits_33", {"max_hits": MAX_HITS + 1})]
    if fam == "shade_rays":
        out += [("no_output", {"pixels": 0, "rgb8": 0, "hits": 0, "status": 0}), ("null_sun", {"sun": 0})]
    if fam == "trace_rays_lists":
        out.append(("null_hits_with_capacity", {"hits": 0}))
    if key == "ray_order":
        out += [("null_rays", {"rays": 0}), ("null_order", {"order": 0}), ("null_scratch", {"scratch": 0}),
                ("rays_misaligned", {"rays": A["rays"] + 4}), ("order_misaligned", {"order": A["order"] + 2}),
                ("scratch_misaligned", {"scratch": A["scratch"] + 4}), ("scratch_small", {"scratch_bytes": A["scratch_bytes"] - 1})]
    elif key == "hit_offsets":
        out += [("null_offsets", {"offsets": 0}), ("offsets_misaligned", {"offsets": A["offsets"] + 4}), ("null_counts", {"counts": 0}),
                ("null_scratch", {"scratch": 0}), ("counts_misaligned", {"counts": A["counts"] + 2}),
                ("scratch_misaligned", {"scratch": A["scratch"] + 4}), ("scratch_small", {"scratch_bytes": A["scratch_bytes"] - 1})]
    else:
        out.append(("null_rays", {"rays": 0}))
    out.append(("n_rays_2_31", {"n": 1 << 31}))
    if key != "hit_offsets":                                          # (its n = 0 is a launch: a one-entry scan)
        out.append(("n_rays_0", {"n": 0}))
    if device:
        out += [("rays_misaligned", {"rays": A["rays"] + 4}), ("hits_misaligned", {"hits": A["hits"] + 4})]
        if fam == "trace_rays_all":
            out.append(("counts_misaligned", {"counts": A["counts"] + 2}))
        if fam == "trace_rays_lists":
            out += [("null_offsets", {"offsets": 0}), ("offsets_misaligned", {"offsets": A["offsets"] + 4})]
        if fam == "shade_rays":
            out.append(("pixels_misaligned", {"pixels": A["pixels"] + 2}))
    if form == "_indexed_device":                                     # check_index_list, after everything above
        out += [("index_stats_scene", {"scene": A["stats_scene"]}), ("index_2_31", {"n_index": 1 << 31}), ("index_empty", {"n_index": 0}),
                ("index_null", {"index": 0}), ("index_misaligned", {"index": A["index"] + 2})]
    return out


SUCCEEDS = ("n_rays_0", "index_empty")                                # successful no-ops; everything else is refused


class Arena:
    """Real buffers for every argument of every call: device tensors for the device calls, numpy arrays for the
    host-array calls, each with slack for the misaligned cases."""

    def __init__(self, gpu, L, f64):
        import torch
        import allhits_common as ac
        import rayorder_common as ro
        import trace64_common as t64
        self.keep = []
        name, other = ("quad_tiny64", "quad_tiny") if f64 else ("quad_tiny", "quad_tiny64")

        def scene(nm, **kw):
            mesh_bvh = t64.ray_set_scene(nm, "exact") if nm.endswith("64") else ac.all_set_scene(nm, 0)
            s = gpu.Scene(*mesh_bvh, **kw)
            self.keep.append(s)
            return s

        self.scenes = {"scene": scene(name)._h, "stats_scene": scene(name, stats=True)._h, "other_scene": scene(other)._h}
        rays = np.ascontiguousarray(ro.set_rays(name)[:N])
        assert len(rays) == N
        hb, pb = (32, 24) if f64 else (16, 12)
        sizes = {"hits": max(N * K, CAP) * hb, "occluded": N, "counts": 4 * N, "offsets": 8 * (N + 1), "pixels": N * pb, "rgb8": 3 * N,
                 "status": N, "counters": 64, "index": 4 * N, "order": 4 * N,
                 "scratch": max(L.ceres_ray_order_scratch_bytes(N), L.ceres_hit_offsets_scratch_bytes(N))}

        def dev(nbytes, src=None):
            t = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
            if src is not None:
                t[:src.nbytes] = torch.from_numpy(src.view(np.uint8).reshape(-1).copy())
            self.keep.append(t)
            return t.data_ptr()

        def host(nbytes, src=None):
            a = np.zeros(nbytes + 64, np.uint8)
            if src is not None:
                a[:src.nbytes] = src.view(np.uint8).reshape(-1)
            self.keep.append(a)
            return a.ctypes.data

        self.sun = (ctypes.c_double * 3 if f64 else ctypes.c_float * 3)(-3, 9, 2.5)
        self.device = {k: dev(v) for k, v in sizes.items()}
        self.device["rays"] = dev(rays.nbytes, rays)
        self.host = {k: host(v) for k, v in sizes.items()}
        self.host["rays"] = host(rays.nbytes, rays)
        self.host["stats"], self.host["total"] = host(64), host(8)
        self.scratch_bytes = {"ray_order": L.ceres_ray_order_scratch_bytes(N), "hit_offsets": L.ceres_hit_offsets_scratch_bytes(N)}
        self.ROBUST = gpu.MODE_ROBUST

    def values(self, key):
        """The valid call's arguments of an entry point."""
        on_host = key == "coherent" or (isinstance(key, tuple) and key[1] == "")
        v = dict(self.host if on_host else self.device)
        v.update(self.scenes)
        v.update(n=N, n_index=N, mode=0, max_hits=K, capacity=CAP, stream=0, sun=ctypes.addressof(self.sun), ROBUST=self.ROBUST,
                 scratch_bytes=self.scratch_bytes.get(key, 0))
        return v

    def close(self):
        for s in self.keep:
            if hasattr(s, "close"):
                s.close()
        self.keep = []


def run_all(gpu):
    """{"<C name>/<case>": [status, message]} of every case on the GPU."""
    import torch
    L, got = open_library(gpu), {}
    arenas = {f64: Arena(gpu, L, f64) for f64 in (False, True)}
    try:
        for key, name, names, f64 in entry_points():
            base = arenas[f64].values(key)
            for case, over in cases_of(key, f64, base):
                res = call(L, name, names, {**base, **over})
                assert (res[0] == 0) == (case in SUCCEEDS), (name, case, res, "refused calls only: nothing may be launched here")
                got[name + "/" + case] = res
        torch.cuda.synchronize()
    finally:
        for a in arenas.values():
            a.close()
    return got


def run_null_scene(pkg):
    """A null scene, every entry point: refused before anything else is looked at (no GPU needed)."""
    L, got = open_library(pkg), {}
    for key, name, names, f64 in entry_points():
        values = {a: 0 for a in names}
        values.update(n=N, n_index=N)
        got[name + "/null_scene"] = call(L, name, names, values)
        assert got[name + "/null_scene"][0] < 0, name
    return got


def compare(got, golden):
    for k, v in got.items():
        assert k in golden, (k, "a case the golden file does not have: record it from the parent build")
        assert v == golden[k], (k, "got", v, "recorded", golden[k])


def load_recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_null_scene_is_refused_with_the_recorded_text(pkg):
    got = run_null_scene(pkg)
    assert len(got) == 29
    compare(got, load_recorded())


@pytest.mark.gpu
def test_refusals_return_the_recorded_status_and_text(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    golden = load_recorded()
    got = run_all(pkg)
    compare(got, golden)
    assert set(got) | set(run_null_scene(pkg)) == set(golden), "a recorded case was not run"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_query_refusals.py --record   (on a GPU, with the parent build's library)")
    from conftest import import_package
    package = import_package()
    recorded = run_null_scene(package)
    recorded.update(run_all(package))
    with open(GOLDEN_FILE, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(recorded), "cases from", package.LIB_PATH)
