#!/usr/bin/env python3
"""Generate tests/golden/soups/soups.json from the REFERENCE's own builder and renderer on the triangle
soups of tests/soup_common.py (NaN, inf, huge and denormal coordinates, which the reference's OBJ loader
cannot produce: they go in as raw bvh::Triangle<float> rows, `ref_render --tri48`).

Runs oracle/_ref/ref_render (reference CMake flags) and oracle/_ref/ref_render_exact (the same with
-ffp-contract=off) and records results only:

  per (kind, n):  the sha256 of the soup's bytes (drift of the generator shows), and per build the node
                  count and the canonical (numbering-independent) sha256 of the BVH
  for soup_common.FRAMES at 97 x 61: the camera (tile_compact_model.look on the finite part's box), the
                  sun, and per build the basis as hex floats, rays / hits and the PPM's sha256, with the
                  fast and with the robust node intersector

A kind on which a reference build crashes or runs past its time limit is listed under "dropped" with
what happened, and has no entry.  Must run where the reference tree exists.
Usage: python tests/golden/make_golden_soups.py"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import oracle  # noqa: E402
import soup_common as sc  # noqa: E402

BUILDS = (("ref", os.path.join(REPO, "oracle", "_ref", "ref_render")),
          ("exact", os.path.join(REPO, "oracle", "_ref", "ref_render_exact")))
SCRATCH = os.path.join(REPO, ".scratch", "golden_soups")
OUT = os.path.join(HERE, "soups", "soups.json")
LIMIT = 120                                      # seconds per reference run


def run(binary, args):
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        raise RuntimeError("exit status %d: %s" % (r.returncode, r.stderr.strip()[-200:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def f3(v):
    return [repr(float(x)) for x in v]


def main():
    os.makedirs(SCRATCH, exist_ok=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    soups, dropped = {}, {}
    p_tri, p_norm = os.path.join(SCRATCH, "soup.tri48"), os.path.join(SCRATCH, "soup.norm36")
    p_dump, p_ppm = os.path.join(SCRATCH, "dump"), os.path.join(SCRATCH, "frame.ppm")
    for kind, n in sc.CASES:
        if kind in dropped:
            continue
        tri, _ = sc.soup(kind, n)
        tri.tofile(p_tri)
        entry = {"tri48_sha256": sc.sha(tri)}
        try:
            for build, binary in BUILDS:
                j = run(binary, ["--tri48", p_tri, "--size", "1", "1", "--dump", p_dump])
                assert j["n_tri"] == n and hashlib.sha256(open(p_dump + ".tri48", "rb").read()).hexdigest() == entry["tri48_sha256"]
                nodes = np.fromfile(p_dump + ".nodes32", dtype=np.uint32).reshape(-1, 8)
                prim = np.fromfile(p_dump + ".prim64", dtype=np.uint64)
                assert nodes.shape[0] == j["n_nodes"]
                entry[build] = {"n_nodes": j["n_nodes"], "bvh_canonical_sha256": oracle.canonical_bvh_sha(nodes, prim)}
        except (RuntimeError, subprocess.TimeoutExpired) as e:
            dropped[kind] = "n = %d, %s" % (n, e)
            for k in [k for k in soups if k.startswith(kind + "-")]:
                del soups[k]
            continue
        soups["%s-%d" % (kind, n)] = entry
        print(kind, n, entry["exact"]["n_nodes"], entry["ref"]["n_nodes"], flush=True)
    frames = {}
    for kind, n in sc.FRAMES:
        if kind in dropped:
            continue
        tri, _ = sc.soup(kind, n)
        tri.tofile(p_tri)
        sc.normals(tri).tofile(p_norm)
        box = sc.finite_box(tri)
        eye, d, up, fov = sc.frame_camera(box)
        sun = sc.sun_of(box)
        frame = {"soup": "%s-%d" % (kind, n), "W": sc.FRAME_W, "H": sc.FRAME_H, "eye": f3(eye), "dir": f3(d), "up": f3(up),
                 "fov": fov, "sun": f3(sun), "norm36_sha256": hashlib.sha256(sc.normals(tri).tobytes()).hexdigest()}
        args = ["--tri48", p_tri, "--norm36", p_norm, "--eye", *f3(eye), "--dir", *f3(d), "--up", *f3(up), "--fov", repr(fov),
                "--sun", *f3(sun), "--size", str(sc.FRAME_W), str(sc.FRAME_H), "--out", p_ppm]
        for build, binary in BUILDS:
            frame[build] = {}
            for name, extra in (("full", []), ("primary", ["--primary-only"]), ("robust", ["--robust"])):
                j = run(binary, args + extra + (["--stats"] if not extra else []))
                e = {"rays": j["rays"], "hits": j["hits"], "ppm_sha256": hashlib.sha256(open(p_ppm, "rb").read()).hexdigest()}
                if name == "full":
                    e["loop_vs_render_mismatch"] = j["loop_vs_render_mismatch"]
                    frame[build]["basis"] = {"dir": j["basis_dir"], "u": j["basis_u"], "v": j["basis_v"]}
                frame[build][name] = e
                os.remove(p_ppm)
        frames[frame["soup"]] = frame
        print("frame", frame["soup"], frame["exact"]["full"], frame["ref"]["full"], flush=True)
    for suf in (".tri48", ".norm36", ".nodes32", ".prim64"):
        if os.path.exists(p_dump + suf):
            os.remove(p_dump + suf)
    meta = {"generator": "oracle/_ref/ref_render{,_exact} --tri48 via tests/golden/make_golden_soups.py",
            "seed": sc.SEED, "dropped": dropped, "soups": soups, "frames": frames}
    with open(OUT, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
