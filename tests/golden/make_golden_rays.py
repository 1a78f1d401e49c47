#!/usr/bin/env python3
"""Generate tests/golden/rays/<set>.npz: caller-style rays and the REFERENCE's own answer to each.

For every ray set of tests/trace_common.py (RAY_SETS) the rays are written to a file of 32-B records
{origin[3], direction[3], tmin, tmax} and traced by the reference's library layer itself --
oracle/ref_harness.cpp's `--rays f --ray-hits g` mode: SingleRayTraverser::traverse(bvh::Ray(o, d,
tmin, tmax), intersector, statistics) (single_ray_traverser.hpp:156-163) with the
ClosestPrimitiveIntersector and then the AnyPrimitiveIntersector (primitive_intersectors.hpp:31-76)
over the scene the harness builds as for frames (OBJ or --proc N, --rotate, BinnedSahBuilder<Bvh, 16>)
-- in the four variants

  exact_fast    oracle/_ref/ref_render_exact            (-ffp-contract=off), FastNodeIntersector
  exact_robust  oracle/_ref/ref_render_exact --robust   RobustNodeIntersector (node_intersectors.hpp:54-79)
  ref_fast      oracle/_ref/ref_render                  (reference CMake flags: FMA contraction)
  ref_robust    oracle/_ref/ref_render --robust

Each variant traces the scene its own build makes (the contracted and the contraction-free scenes
differ in bits).  One file per set:

  rays                  float32 [n, 8], the input, as stored bits
  <variant>_prim        int32   hit->primitive_index, -1 on a miss
  <variant>_t, _u, _v   uint32  the bits of hit->intersection.{t, u, v}, 0 on a miss
  <variant>_occluded    uint8   the any-hit walk found a hit
  <variant>_steps       uint32  Statistics::traversal_steps of the closest walk
  <variant>_tests       uint32  Statistics::intersections of the closest walk

The double sets of tests/trace64_common.py (RAY_SETS64) go to tests/golden/rays64/<set>.npz the same
way: 64-B rays of 8 doubles through oracle/_ref/ref_render_f64_exact (exact_fast) and ref_render_f64
(ref_fast) -- the product's double path has no robust mode -- whose 40-B records are {int32 prim,
int32 occluded, double t, u, v, uint32 steps, uint32 tests}; `rays` is float64 [n, 8] and `_t, _u, _v`
are uint64 bits.  dragon_adversarial64 is stored whole (4,099 rays, under the size limit).

lattice_ties and lattice_ties64 must meet the floors of trace_common.check_lattice_conditions on
their stored outputs (boundary hits by the score, coincident twins, variants that agree or differ as
stated); a draw that falls short fails here.

The archives are written with fixed member dates, so a rerun reproduces them byte for byte.  Needs
the built package (the sets' rays come from its scenes) and `make -C oracle ref`; the tests read only
the stored files.
Usage: python tests/golden/make_golden_rays.py [set ...]     (default: every float and double set)
"""
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import trace_common as tc  # noqa: E402  (puts the package directory on sys.path)
import trace64_common as t64  # noqa: E402
import configs  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "ref_render")
REF_EXACT = os.path.join(REPO, "oracle", "_ref", "ref_render_exact")
VARIANTS = {"exact_fast": (REF_EXACT, []), "exact_robust": (REF_EXACT, ["--robust"]),
            "ref_fast": (REF, []), "ref_robust": (REF, ["--robust"])}
SCRATCH = os.path.join(REPO, ".scratch", "golden_rays")
OUT = os.path.join(HERE, "rays")
MAX_BYTES = 1 << 20

REF64 = os.path.join(REPO, "oracle", "_ref", "ref_render_f64")
REF64_EXACT = os.path.join(REPO, "oracle", "_ref", "ref_render_f64_exact")
VARIANTS64 = {"exact_fast": (REF64_EXACT, []), "ref_fast": (REF64, [])}
OUT64 = os.path.join(HERE, "rays64")
HIT64_DTYPE = np.dtype([("prim", "<i4"), ("occluded", "<i4"), ("t", "<u8"), ("u", "<u8"), ("v", "<u8"), ("steps", "<u4"),
                        ("tests", "<u4")])
assert HIT64_DTYPE.itemsize == 40

HIT_DTYPE = np.dtype([("prim", "<i4"), ("t", "<u4"), ("u", "<u4"), ("v", "<u4"), ("occluded", "<i4"), ("steps", "<u4"),
                      ("tests", "<u4")])


def save_npz(path, arrays):
    """np.savez_compressed's format with every member dated 1980-01-01: the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def make(name):
    f64 = name in t64.RAY_SETS64
    mod, out, variants, hit_dtype, real = (t64, OUT64, VARIANTS64, HIT64_DTYPE, np.float64) if f64 else \
        (tc, OUT, VARIANTS, HIT_DTYPE, np.float32)
    os.makedirs(SCRATCH, exist_ok=True)
    os.makedirs(out, exist_ok=True)
    rays = np.ascontiguousarray(mod.ray_set_rays(name), real)
    cfg = dict(mod.ray_set_config(name), robust=False, mode="full", orbit=None)
    p_rays = os.path.join(SCRATCH, name + ".rays.bin")
    rays.tofile(p_rays)
    arrays = {"rays": rays}
    summary = {}
    for variant, (binary, extra) in variants.items():
        p_hits = os.path.join(SCRATCH, "%s.%s.hits.bin" % (name, variant))
        cmd = [binary] + configs.cli_args(cfg) + extra + ["--rays", p_rays, "--ray-hits", p_hits]
        j = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
        rec = np.fromfile(p_hits, dtype=hit_dtype)
        assert rec.size == len(rays) == j["rays"], (name, variant)
        miss = rec["prim"] < 0
        assert not (rec["t"][miss] | rec["u"][miss] | rec["v"][miss]).any()
        for k in ("prim", "t", "u", "v", "steps", "tests"):
            arrays[variant + "_" + k] = rec[k]
        arrays[variant + "_occluded"] = rec["occluded"].astype(np.uint8)
        summary[variant] = (int((~miss).sum()), int(rec["occluded"].sum()))
        os.remove(p_hits)
    os.remove(p_rays)
    path = os.path.join(out, name + ".npz")
    save_npz(path, arrays)
    assert os.path.getsize(path) <= MAX_BYTES, (path, os.path.getsize(path))
    print(name, len(rays), "rays;", ", ".join("%s %d hits %d occluded" % ((v,) + summary[v]) for v in variants),
          "; %d bytes" % os.path.getsize(path), flush=True)
    if name in (tc.LATTICE, t64.LATTICE64):
        fx = t64.load_ray_fixture64(name) if f64 else tc.load_ray_fixture(name)
        print(" ", tc.check_lattice_conditions(fx, robust=not f64), flush=True)


if __name__ == "__main__":
    for n in sys.argv[1:] or tc.RAY_SETS + t64.RAY_SETS64:
        make(n)
