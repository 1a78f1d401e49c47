#!/usr/bin/env python3
"""tests/golden/deep/cap26.json: the reference's answers on cap26 (tests/deep_common.py: 2,600
triangles whose BVH reaches the builder's depth cap of 64 levels).

The mesh is not committed -- its OBJ text is regenerated and held to a sha256 -- so the scene is
not a configs.CONFIGS entry; its views (deep_common.CAP26_VIEWS) are rendered here by
oracle/_ref/ref_render (reference CMake flags) and ref_render_exact (-ffp-contract=off) exactly as
make_golden.py renders a config, and one JSON keeps, per build, the scene hashes and per view the
camera basis and pose bits, the PPM's sha256, rays / hits, the traversal Statistics and a seeded
sample of the per-pixel records {pixel, prim, t, u, v bits, shadow}.
Usage: python tests/golden/make_golden_deep.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import deep_common as dc  # noqa: E402
import make_golden as mg  # noqa: E402

SAMPLE_HITS, SAMPLE_OTHER, SEED = 384, 64, 12345


def main():
    os.makedirs(os.path.join(HERE, "deep"), exist_ok=True)
    out = {"mesh": "cap26", "obj_sha256": dc.CAP26_SHA256,
           "generator": "oracle/_ref/ref_render{,_exact} via tests/golden/make_golden_deep.py", "views": {}}
    with tempfile.TemporaryDirectory() as tmp:
        obj = dc.obj_path("cap26", tmp)
        for view in dc.CAP26_VIEWS:
            cfg = dc.cap26_cfg(view, obj)
            W, H = cfg["W"], cfg["H"]
            entry = {}
            for build, binary in (("ref", mg.REF), ("exact", mg.REF_EXACT)):
                p = os.path.join(tmp, "%s.%s" % (view, build))
                j = mg.run(binary, cfg, ["--out", p + ".ppm", "--stats", "--records", p + ".rec", "--dump", p])
                rec = np.fromfile(p + ".rec", dtype=mg.REC_DTYPE)
                assert rec.size == W * H
                dc.check_view(rec["prim"], rec["shadow"], cfg["mode"])
                scene = mg._scene_hashes(p)
                scene.update(n_tri=j["n_tri"], n_nodes=j["n_nodes"])
                assert out.setdefault("scene_" + build, scene) == scene
                rng = np.random.default_rng(SEED)
                hit, other = np.flatnonzero(rec["prim"] >= 0), np.flatnonzero(rec["prim"] < 0)
                keep = np.sort(np.concatenate([rng.choice(hit, min(SAMPLE_HITS, hit.size), replace=False),
                                               rng.choice(other, min(SAMPLE_OTHER, other.size), replace=False)]))
                r = rec[keep]
                entry[build] = {
                    "rays": j["rays"], "hits": j["hits"], "stats": {k: j[k] for k in mg.STAT_KEYS},
                    "basis": j["basis_dir"] + j["basis_u"] + j["basis_v"], "eye": j["eye"], "sun": j["sun"],
                    "ppm_sha256": mg.sha(p + ".ppm"),
                    "records": {"pixel": (r["j"].astype(np.int64) * W + r["i"]).tolist(), "prim": r["prim"].tolist(),
                                "shadow": r["shadow"].tolist(),
                                "tuv_bits": np.stack([r["t"], r["u"], r["v"]], 1).view(np.uint32).ravel().tolist()},
                }
            out["views"][view] = entry
            print(view, entry["exact"]["rays"], entry["exact"]["hits"], entry["ref"]["hits"], flush=True)
    path = os.path.join(HERE, "deep", "cap26.json")
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
