"""Shared pieces of the complete-hit-list tests (test_hitlists_cpu.py, test_gpu_hitlists.py).

The complete-hit-list query returns the hit sets of the all-hits query (allhits_common.py) without a cap, as a
CSR pair: offsets [n + 1] u64, the exclusive prefix sums of the per-ray counts, and offsets[n] hit16 records,
ray r owning [offsets[r], offsets[r + 1]) -- its whole set in the key order (t by float <, equal t with
-0 == +0 by original triangle index).  Every path is a `trace_lists(rays, mode) -> (offsets, hits, stats)`
callable here.

The reference's own answer lies in tests/golden/rays_lists/ (tests/golden/make_golden_hitlists.py): its
traverser's collecting run as in rays_all/, stored whole."""
import functools
import os

import numpy as np

import allhits_common as ac
import trace_common as tc
from conftest import GOLDEN

F = np.float32
LIST_DIR = os.path.join(GOLDEN, "rays_lists")
SOUP_LONG = "soup_mixed_nan_4097"
# set -> the first n rays of tests/golden/rays_all/<set>'s rays (None: all of them)
LIST_SETS = {ac.DUPLEAF: None, "arms6_centroids": None, "bodyarms_centroids": None, "soup_nan_p0_300": None, SOUP_LONG: 128,
             tc.LATTICE: None, "tri1_tiny": None}
ENOMEM, EINVAL, EHIP, ESTACK, EUNSUPPORTED = -3, -1, -4, -5, -6


def sort_whole(counts, rec):
    """allhits_common.sort_and_truncate without the cut: the walk-order records `rec` (structured, ray after
    ray, counts[k] each) after a stable sort per ray by (t by float <, original triangle index)."""
    ray = np.repeat(np.arange(len(counts)), counts.astype(np.int64))
    t = rec["t"].view(F)
    assert not np.isnan(t).any()
    return rec[np.lexsort((rec["prim"], t, ray))]                     # stable; float keys compare -0 == +0


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)


def list_rays(name):
    """The rays a set's stored lists belong to."""
    return np.ascontiguousarray(ac.load_all_fixture(name)["rays"][:LIST_SETS[name]])


@functools.lru_cache(maxsize=None)
def load_list_fixture(name):
    """tests/golden/rays_lists/<name>.npz (or <name>.<variant>.npz): {"rays", variant: {"count" uint32 [n],
    "offsets" uint64 [n + 1], "hits" HIT_DTYPE [total], "steps", "tests" uint32 [n] (those of rays_all/)}};
    read-only, loaded once; the rays' sha256 is verified."""
    one = os.path.join(LIST_DIR, name + ".npz")
    files = [np.load(one)] if os.path.exists(one) else [np.load(os.path.join(LIST_DIR, "%s.%s.npz" % (name, v))) for v in tc.RAY_VARIANTS]
    z = {k: f[k] for f in files for k in f.files}
    rays = list_rays(name)
    assert bytes(z["rays_sha256"]).decode() == ac.rays_sha256(rays), name
    allfx = ac.load_all_fixture(name)
    out = {"rays": rays}
    for v in tc.RAY_VARIANTS:
        count = z[v + "_count"]
        assert count.shape == (len(rays),) and len(z[v + "_prim"]) == int(count.sum(dtype=np.uint64))
        hits = np.zeros(len(z[v + "_prim"]), ac.HIT_DTYPE)
        hits["prim"] = z[v + "_prim"]
        for k in ("t", "u", "v"):
            hits[k] = z[v + "_" + k].view(F)
        out[v] = {"count": count, "offsets": offsets_of(count), "hits": hits,
                  "steps": allfx[v]["steps"][:len(rays)], "tests": allfx[v]["tests"][:len(rays)]}
    for a in [out["rays"]] + [a for v in tc.RAY_VARIANTS for a in out[v].values()]:
        a.setflags(write=False)
    return out


def check_list_fixture_floors():
    """What the stored lists are there for, on the reference's answers alone: over a hundred rays past 32 hits
    in each exact variant of the two centroid sets, a 987-hit ray in the soup subset, a 170-hit ray of two t
    values on dupleaf_stack, a 32-hit ray and none longer on lattice_ties."""
    for name in ("arms6_centroids", "bodyarms_centroids"):
        for v in ("exact_fast", "exact_robust"):
            assert (load_list_fixture(name)[v]["count"] > ac.MAX_HITS).sum() >= 100, (name, v)
    assert max(int(load_list_fixture(SOUP_LONG)[v]["count"].max()) for v in tc.RAY_VARIANTS) == 987
    for v in tc.RAY_VARIANTS:
        fx = load_list_fixture(ac.DUPLEAF)[v]
        k = int(np.argmax(fx["count"]))
        assert fx["count"][k] >= 170, v
        seg = fx["hits"][int(fx["offsets"][k]):int(fx["offsets"][k + 1])]
        assert len(np.unique(seg["t"][:170])) == 2, v
    assert max(int(load_list_fixture(tc.LATTICE)[v]["count"].max()) for v in tc.RAY_VARIANTS) <= ac.MAX_HITS
    assert int(load_list_fixture("tri1_tiny")["exact_fast"]["count"].max()) == 1


def hits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_bad_ray(offsets, got, exp):
    """The first ray whose segment differs (for messages)."""
    bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != exp.view(np.uint32).reshape(-1, 4)).any(axis=1))
    return None if not len(bad) else int(np.searchsorted(offsets, bad[0], side="right") - 1)


def check_against_list_fixture(pkg, trace_lists, name, variant, stats):
    """trace_lists on the set's scene prepared for `variant` returns the reference's complete lists bit for
    bit, offsets = [0] + cumsum(counts), stats rays / hits; with `stats` (the CPU path, GPU stats scenes)
    node_pairs / tri_tests are the reference's summed Statistics, the NaN rays in a call of their own as in
    allhits_common.check_against_all_fixture."""
    fx = load_list_fixture(name)
    ref = fx[variant]
    mode, _ = tc.variant_mode(pkg, variant)
    idx = np.arange(len(fx["rays"]))
    parts = [idx]
    if stats:
        nan = np.isnan(fx["rays"]).any(axis=1)
        parts = [idx[~nan]] + ([idx[nan]] if nan.any() else [])
    for k, part in enumerate(parts):
        where = (name, variant, "stats" if stats else "production", "part %d" % k)
        rays = np.ascontiguousarray(fx["rays"][part])
        cnt = ref["count"][part]
        exp = np.concatenate([ref["hits"][int(ref["offsets"][r]):int(ref["offsets"][r + 1])] for r in part]) if len(part) else ref["hits"][:0]
        off, hits, st = trace_lists(rays, mode)
        assert off.dtype == np.uint64 and np.array_equal(off, offsets_of(cnt)), (where, "offsets")
        assert hits.dtype == pkg.HIT_DTYPE and len(hits) == len(exp), where
        assert hits_equal(hits, exp), (where, "first differing ray", part[first_bad_ray(off, hits, exp)])
        assert st["rays"] == len(part) and st["hits"] == int((cnt >= 1).sum()), where
        if stats:
            assert st["node_pairs"] == int(ref["steps"][part].sum(dtype=np.uint64)), where
            assert st["tri_tests"] == int(ref["tests"][part].sum(dtype=np.uint64)), where


def check_lists(rays, offsets, hits):
    """A CSR answer is well formed: offsets non-decreasing from 0 to len(hits); every record a real hit with
    t inside its ray's window; each segment strictly increasing in the key (so prims are distinct)."""
    n = len(rays)
    assert offsets.shape == (n + 1,) and offsets.dtype == np.uint64 and offsets[0] == 0 and offsets[n] == len(hits)
    counts = np.diff(offsets.astype(np.int64))
    assert (counts >= 0).all()
    ray = np.repeat(np.arange(n), counts)
    t, p = hits["t"], hits["prim"]
    assert (p >= 0).all() and not np.isnan(t).any()
    assert ((t >= rays[ray, 6]) & (t <= rays[ray, 7])).all()
    same = ray[1:] == ray[:-1]
    a, b, pa, pb = t[:-1], t[1:], p[:-1], p[1:]
    assert ((a < b) | ((a == b) & (pa < pb)))[same].all()


def check_against_trace_all(trace_lists, trace_all, rays, mode):
    """Against the capped query: counts equal; each list's first min(count, 32) records are the max_hits = 32
    row; and check_lists.  Returns (offsets, hits)."""
    rays = np.ascontiguousarray(rays)
    off, hits, st = trace_lists(rays, mode)
    counts, rows, st32 = trace_all(rays, ac.MAX_HITS, mode, True)
    check_lists(rays, off, hits)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts.astype(np.int64))
    assert (st["rays"], st["hits"]) == (st32["rays"], st32["hits"]) == (len(rays), int((counts >= 1).sum()))
    kept = np.minimum(counts, ac.MAX_HITS).astype(np.int64)
    real = np.arange(ac.MAX_HITS)[None, :] < kept[:, None]
    src = (off[:-1].astype(np.int64)[:, None] + np.arange(ac.MAX_HITS)[None, :])[real]
    assert hits_equal(np.ascontiguousarray(hits[src]), np.ascontiguousarray(rows[real]))
    return off, hits
