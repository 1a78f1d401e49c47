#!/usr/bin/env python3
"""Generate tests/golden/rays_lists/<set>.npz: the COMPLETE hit list of every ray, as the reference's own
traverser found it -- what the complete-hit-list query (ceres_trace_rays_lists*) must return.

The run is make_golden_allhits.py's: each ray once through SingleRayTraverser::traverse with the collecting
intersector of oracle/ref_harness.cpp (`--rays f --ray-all-hits g --ray-all-counts c`), in the four variants
of make_golden_rays.VARIANTS.  The harness writes every hit of every ray, in walk order and of variable
length; here nothing is cut off at 32: the records are stored whole after a stable sort by the product's key
(t by float <, equal t with -0 == +0 by original triangle index).

The sets (hitlists_common.LIST_SETS: set -> the first n rays of tests/golden/rays_all/<set>'s rays, None =
all), chosen so that each file stays within make_golden_rays.MAX_BYTES: dupleaf_stack (runs of 130 and 40
equal t), arms6_centroids and bodyarms_centroids (real meshes, deep trees, over a hundred rays past 32
hits), soup_nan_p0_300 (NaN soup), the first 128 rays of soup_mixed_nan_4097 (a 987-hit ray, the largest
set of the repository), lattice_ties (the old cap's boundary) and tri1_tiny (a root-leaf scene).

One file per set (one per variant, <set>.<variant>.npz, where a single file would pass the limit):

  rays_sha256            uint8   the hex sha256 of the float32 [n, 8] rays the answers belong to
  <variant>_count        uint32 [n]  the size of each ray's hit set
  <variant>_prim         int32   every record, ray after ray in key order; offsets are cumsum(count)
  <variant>_t, _u, _v    uint32  ... as bits

Asserted here, on the reference's output alone: the counts are those stored in tests/golden/rays_all/; the
first min(count, 32) records of each sorted list are the stored rays_all row; and the floors of
hitlists_common.check_list_fixture_floors.  The archives are written by make_golden_rays.save_npz: a rerun
reproduces them byte for byte.  Needs `make -C oracle ref` only, not the built package.
Usage: python tests/golden/make_golden_hitlists.py [set ...]     (default: every set)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import allhits_common as ac  # noqa: E402  (puts the package directory on sys.path)
import hitlists_common as hc  # noqa: E402
from make_golden_allhits import ALL_DTYPE, COUNT_DTYPE, run, scene_args  # noqa: E402
from make_golden_rays import MAX_BYTES, VARIANTS, save_npz  # noqa: E402

SCRATCH = os.path.join(REPO, ".scratch", "golden_hitlists")


def make(name):
    os.makedirs(SCRATCH, exist_ok=True)
    os.makedirs(hc.LIST_DIR, exist_ok=True)
    stored = ac.load_all_fixture(name)
    first = hc.LIST_SETS[name]
    rays = np.ascontiguousarray(stored["rays"][:first], np.float32)
    n = len(rays)
    p_rays, p_hits, p_counts = (os.path.join(SCRATCH, name + s) for s in (".rays.bin", ".hits.bin", ".counts.bin"))
    rays.tofile(p_rays)
    scene = scene_args(name, SCRATCH)
    head = {"rays_sha256": np.frombuffer(ac.rays_sha256(rays).encode(), np.uint8)}
    per_variant, summary = {}, {}
    for variant, (binary, extra) in VARIANTS.items():
        j = run([binary] + scene + extra + ["--rays", p_rays, "--ray-all-hits", p_hits, "--ray-all-counts", p_counts])
        cnt = np.fromfile(p_counts, dtype=COUNT_DTYPE)
        rec = np.fromfile(p_hits, dtype=ALL_DTYPE)
        assert cnt.size == n == j["rays"] and rec.size == int(cnt["count"].sum(dtype=np.uint64)) == j["hits"], (name, variant)
        ref = stored[variant]
        assert np.array_equal(cnt["count"], ref["count"][:n]), (name, variant)
        assert np.array_equal(cnt["steps"], ref["steps"][:n]) and np.array_equal(cnt["tests"], ref["tests"][:n]), (name, variant)
        full = hc.sort_whole(cnt["count"], rec)
        start = np.concatenate([[0], np.cumsum(cnt["count"].astype(np.int64))])
        for k in range(n):                                            # the stored row is the list's head
            m = min(int(cnt["count"][k]), ac.MAX_HITS)
            head_k, row = full[start[k]:start[k] + m], ref["rows"][k, :m]
            assert all(np.array_equal(head_k[f].view(np.uint32), row[f].view(np.uint32)) for f in ac.HIT_FIELDS), (name, variant, k)
        arrays = {variant + "_count": cnt["count"]}
        arrays.update({variant + "_" + f: full[f] for f in ac.HIT_FIELDS})
        per_variant[variant] = arrays
        summary[variant] = "%d records, most %d, %d rays past %d" % (
            len(full), int(cnt["count"].max()), int((cnt["count"] > ac.MAX_HITS).sum()), ac.MAX_HITS)
        os.remove(p_hits)
        os.remove(p_counts)
    os.remove(p_rays)
    if name in ac.SOUP_SETS:
        os.remove(os.path.join(SCRATCH, name + ".tri48"))
    for v in VARIANTS:
        stale = os.path.join(hc.LIST_DIR, "%s.%s.npz" % (name, v))
        if os.path.exists(stale):
            os.remove(stale)
    one = os.path.join(hc.LIST_DIR, name + ".npz")
    merged = dict(head)
    for v in VARIANTS:
        merged.update(per_variant[v])
    save_npz(one, merged)
    paths = [one]
    if os.path.getsize(one) > MAX_BYTES:                              # one file per variant instead
        os.remove(one)
        paths = []
        for k, v in enumerate(VARIANTS):
            paths.append(os.path.join(hc.LIST_DIR, "%s.%s.npz" % (name, v)))
            save_npz(paths[-1], dict(head if k == 0 else {}, **per_variant[v]))
    for p in paths:
        assert os.path.getsize(p) <= MAX_BYTES, (p, os.path.getsize(p))
    print(name, n, "rays;", "%d bytes in %d file(s)" % (sum(os.path.getsize(p) for p in paths), len(paths)), flush=True)
    for v in VARIANTS:
        print("  %-12s %s" % (v, summary[v]), flush=True)


if __name__ == "__main__":
    names = sys.argv[1:] or list(hc.LIST_SETS)
    for s in names:
        make(s)
    if set(hc.LIST_SETS) <= set(names):
        hc.load_list_fixture.cache_clear()
        hc.check_list_fixture_floors()
        print("floors hold", flush=True)
