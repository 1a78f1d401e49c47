#!/usr/bin/env python3
"""Generate tests/golden/rays_all/<set>.npz: every hit the REFERENCE's own traverser finds in a ray's window.

Each ray goes once through SingleRayTraverser::traverse(ray, intersector, statistics)
(single_ray_traverser.hpp:156-163) with the collecting intersector of oracle/ref_harness.cpp
(`--rays f --ray-all-hits g --ray-all-counts c`): any_hit = false, every accepted primitive appended to the
ray's own vector, and a Result whose distance() is ray.tmax, so the walk never narrows the window.  The four
variants are those of make_golden_rays.py (exact / reference-flag build x Fast / Robust node intersector),
each over the scene its own build makes.

The sets: the eight of trace_common.RAY_SETS, whose rays are read from tests/golden/rays/<set>.npz (the file
made here stores their sha256, not the rays), and the new sets of allhits_common.py, whose rays are stored --
dupleaf_stack (config dupleaf: leaves of 130 and 40 coincident triangles) and soup_<kind>_<n> for the four
soups of soup_common.RENDERED, which reach the harness as raw rows through --tri48.

One file per set (one per variant, <set>.<variant>.npz, where a single file would pass 1 MiB):

  rays_sha256            uint8   the hex sha256 of the float32 [n, 8] rays the answers belong to
  rays                   float32 [n, 8], new sets only
  <variant>_count        uint32 [n]  hits the walk presented
  <variant>_steps        uint32 [n]  Statistics::traversal_steps
  <variant>_tests        uint32 [n]  Statistics::intersections
  <variant>_prim         int32   ragged: per ray the first min(count, 32) records after a stable sort of the
  <variant>_t, _u, _v    uint32  walk-order records by (t by float <, original triangle index); offsets are
                                 cumsum(min(count, 32)); t, u, v as bits

Asserted here, on the reference's output alone: count >= 1 exactly where the closest / any-hit walks of the
same binary report a hit (the stored <variant>_occluded of tests/golden/rays/ for the existing sets, a
--ray-hits run for the new ones); that closest record is in the row wherever count <= 32; the summed steps
and tests equal the harness's JSON line; and the floors of allhits_common.check_all_fixture_floors (rays
past 32, 40 and 130 hits on dupleaf_stack, rows of several hits and empty rows on the soups).  What each
soup gives is printed; `huge` is ONE leaf of 4,097 triangles (soup_common: an infinite root diagonal), so
every ray tests them all with no box in the way and steps are 0.

The archives are written by make_golden_rays.save_npz: a rerun reproduces them byte for byte.  Needs
`make -C oracle ref` only, not the built package.
Usage: python tests/golden/make_golden_allhits.py [set ...]     (default: every set)
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import allhits_common as ac  # noqa: E402  (puts the package directory on sys.path)
import soup_common  # noqa: E402
import trace_common as tc  # noqa: E402
import configs  # noqa: E402
from make_golden_rays import HIT_DTYPE, MAX_BYTES, VARIANTS, save_npz  # noqa: E402

SCRATCH = os.path.join(REPO, ".scratch", "golden_allhits")
ALL_DTYPE = np.dtype([("prim", "<i4"), ("t", "<u4"), ("u", "<u4"), ("v", "<u4")])
COUNT_DTYPE = np.dtype([("count", "<u4"), ("steps", "<u4"), ("tests", "<u4")])

# the configs of the existing sets, without the package: trace_common.ray_set_config imports it
_PROC300 = dict(configs.CONFIGS["proc_101"], proc=300)
_LATTICE = dict(configs.CONFIGS["quad"], obj="@golden/lattice.obj")


def scene_args(name, scratch):
    """The harness's scene flags for a set."""
    if name in ac.SOUP_SETS:
        tri, _ = soup_common.soup(*ac.SOUP_SETS[name])
        p = os.path.join(scratch, name + ".tri48")
        tri.tofile(p)
        return ["--tri48", p]
    cfg = configs.CONFIGS["dupleaf"] if name == ac.DUPLEAF else _PROC300 if name == "proc300_window" else \
        _LATTICE if name == tc.LATTICE else configs.CONFIGS[tc._SET_CONFIG[name]]
    return configs.cli_args(dict(cfg, robust=False, mode="full", orbit=None))


def run(cmd):
    return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])


def make(name):
    os.makedirs(SCRATCH, exist_ok=True)
    os.makedirs(ac.ALL_DIR, exist_ok=True)
    new = name in ac.NEW_SETS
    stored = None if new else tc.load_ray_fixture(name)
    rays = np.ascontiguousarray(ac.new_set_rays(name) if new else stored["rays"], np.float32)
    n = len(rays)
    p_rays, p_hits, p_counts = (os.path.join(SCRATCH, name + s) for s in (".rays.bin", ".hits.bin", ".counts.bin"))
    rays.tofile(p_rays)
    scene = scene_args(name, SCRATCH)
    head = {"rays_sha256": np.frombuffer(ac.rays_sha256(rays).encode(), np.uint8)}
    if new:
        head["rays"] = rays
    per_variant, summary = {}, {}
    for variant, (binary, extra) in VARIANTS.items():
        j = run([binary] + scene + extra + ["--rays", p_rays, "--ray-all-hits", p_hits, "--ray-all-counts", p_counts])
        cnt = np.fromfile(p_counts, dtype=COUNT_DTYPE)
        rec = np.fromfile(p_hits, dtype=ALL_DTYPE)
        assert cnt.size == n == j["rays"] and rec.size == int(cnt["count"].sum(dtype=np.uint64)) == j["hits"], (name, variant)
        assert int(cnt["steps"].sum(dtype=np.uint64)) == j["steps"] and int(cnt["tests"].sum(dtype=np.uint64)) == j["tests"], (name, variant)
        kept = ac.sort_and_truncate(cnt["count"], rec)
        assert len(kept) == int(np.minimum(cnt["count"], ac.MAX_HITS).sum())
        # the closest and any-hit walks of the same binary: the stored answers, or a run of --ray-hits
        if new:
            run([binary] + scene + extra + ["--rays", p_rays, "--ray-hits", p_hits])
            closest = np.fromfile(p_hits, dtype=HIT_DTYPE)
        else:
            closest = stored[variant]
        occ = np.asarray(closest["occluded"]).astype(bool)
        assert np.array_equal(cnt["count"] >= 1, occ), (name, variant, np.flatnonzero((cnt["count"] >= 1) != occ)[:8])
        assert np.array_equal(np.asarray(closest["prim"]) >= 0, occ), (name, variant)
        start = np.concatenate([[0], np.cumsum(np.minimum(cnt["count"], ac.MAX_HITS).astype(np.int64))])
        for k in np.flatnonzero(occ & (cnt["count"] <= ac.MAX_HITS)):
            row = kept[start[k]:start[k + 1]]
            want = tuple(int(closest[f][k]) for f in ac.HIT_FIELDS)
            assert any(tuple(int(x) for x in h) == want for h in row), (name, variant, int(k))
        arrays = {variant + "_" + f: cnt[f] for f in ("count", "steps", "tests")}
        arrays.update({variant + "_" + f: kept[f] for f in ac.HIT_FIELDS})
        per_variant[variant] = arrays
        summary[variant] = "%d rays hit, %d hits, most %d, %d rows past %d, steps %d, tests %d" % (
            int((cnt["count"] >= 1).sum()), j["hits"], int(cnt["count"].max()), int((cnt["count"] > ac.MAX_HITS).sum()), ac.MAX_HITS,
            j["steps"], j["tests"])
        os.remove(p_hits)
        os.remove(p_counts)
    os.remove(p_rays)
    if name in ac.SOUP_SETS:
        os.remove(os.path.join(SCRATCH, name + ".tri48"))
    for v in VARIANTS:
        stale = os.path.join(ac.ALL_DIR, "%s.%s.npz" % (name, v))
        if os.path.exists(stale):
            os.remove(stale)
    one = os.path.join(ac.ALL_DIR, name + ".npz")
    merged = dict(head)
    for v in VARIANTS:
        merged.update(per_variant[v])
    save_npz(one, merged)
    paths = [one]
    if os.path.getsize(one) > MAX_BYTES:                              # one file per variant instead
        os.remove(one)
        paths = []
        for k, v in enumerate(VARIANTS):
            paths.append(os.path.join(ac.ALL_DIR, "%s.%s.npz" % (name, v)))
            save_npz(paths[-1], dict(head if k == 0 else {}, **per_variant[v]))
    for p in paths:
        assert os.path.getsize(p) <= MAX_BYTES, (p, os.path.getsize(p))
    print(name, n, "rays;", "%d bytes in %d file(s)" % (sum(os.path.getsize(p) for p in paths), len(paths)), flush=True)
    for v in VARIANTS:
        print("  %-12s %s" % (v, summary[v]), flush=True)


if __name__ == "__main__":
    names = sys.argv[1:] or ac.ALL_SETS
    for s in names:
        make(s)
    if set(ac.ALL_SETS) <= set(names):
        ac.load_all_fixture.cache_clear()
        ac.check_all_fixture_floors()
        print("floors hold", flush=True)
