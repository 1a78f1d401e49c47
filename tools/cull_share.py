#!/usr/bin/env python3
"""How much of a bench step the background cull removes from the tile order: for the F views of
bench.py's step (pkg.bench_views) of a config, the 8x8 tiles and pixels whose rays cull_rect proves
to miss the root box (tests/cull_fill_model.py restates cull_rect and the kernels' tile test), and
the fill path's store instructions for them (16 B per lane, 64 lanes, heads and tails included)
next to the tile path's (one 12-B float piece and three RGB8 bytes per lane and tile).  Also the
entry nodes of the same launch (csrc/entry_cut.hpp, through the host entry points): the kept tiles
that no cut rectangle reaches (empty S: nothing walked) and the histogram of the depth at which
the others' primary walks start (0: the root).  "retire": the launch's retired tiles (root-culled or
empty S: the fill workgroups'), the kept groups whose wavefronts leave at once (every tile
retired), the groups left working, and the fill path's column runs (tests/retire_model.py).  No GPU.

usage: python tools/cull_share.py [config] [frames] [orbit|config]   -> one JSON line
(orbit: the step's orbit views; config: F copies of the config's own view, bench.py's default step)
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import import_package  # noqa: E402
import cull_fill_model as M  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "dragon_1080"
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    sys.path.insert(0, REPO)
    import bench
    pkg = import_package()
    cfg = pkg.configs.CONFIGS[name]
    W, H = cfg["W"], cfg["H"]
    mesh, bvh, cam = pkg.prepare(cfg, arith=pkg.ARITH_FMA)
    meta = bench.load_golden(name)
    b12, _, _ = pkg.bench_views(cam, cfg["sun"], W, H, F, basis0=bench.pinned_basis(meta, cfg, cam, "ref"))
    views = sys.argv[3] if len(sys.argv) > 3 else "orbit"
    if views == "config":
        b12 = [b12[0]] * F
    root = M.root_box(mesh.tri)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    tiles = culled = px_culled = fill_instr = 0
    t = M.whole(H)
    import numpy as np
    pairs, _, rlc = pkg.entry_relayout(mesh, bvh)
    cut = pkg.entry_cut(pairs, rlc, bvh.nodes[0, :6].copy().view(np.float32))
    depth_of = {int(cut.lca[i, j]): int(cut.depth[i, j]) for i in range(cut.n) for j in range(cut.n)}
    depth_of[0] = 0
    empty_s, depth_hist = 0, {}
    for f in range(F):
        r = M.cull_rect(b12[f], root, W, H)
        entry = pkg.entry_tiles(cut, pkg.entry_rects(cut, b12[f], W, H), W, H)
        for by in range(ty):
            hit = M.rows_hit(by, 0, r, H, H, t)
            rows = min(8, H - 8 * by)
            for bx in range(tx):
                tiles += 1
                if M.tile_misses_root(r, W, bx, hit):
                    culled += 1
                    px_culled += rows * min(8, W - 8 * bx)
                elif entry[by, bx] == pkg.ENTRY_EMPTY:
                    empty_s += 1
                else:
                    d = depth_of[int(entry[by, bx])]
                    depth_hist[d] = depth_hist.get(d, 0) + 1
        fl, rg = M.fill_runs(r, W, H, t)
        for runs, size in ((fl, 4), (rg, 1)):
            for s, n in runs:
                head, nv, tail = M.zero_run_pieces(s * size, n, size)
                fill_instr += (head > 0) + (nv + 63) // 64 + (tail > 0)
    # the wavefront groups of the batch order (tiles per wave: 2 for 16-bit-stack scenes at 1-4 Mpixel,
    # else 4) whose tiles are all culled: what a compacted order drops (pkg.kept_tiles, the host's count)
    tpw = int(sys.argv[4]) if len(sys.argv) > 4 else (2 if (1 << 20) <= W * H < (1 << 22) else 4)
    groups = (tiles + tpw - 1) // tpw
    empty = None
    if 2 <= F <= 56:
        kept = pkg.kept_tiles(W, H, F, tpw, [list(M.cull_rect(b12[f], root, W, H)) for f in range(F)])["tiles"]
        empty = groups - (kept + tpw - 1) // tpw
    # Retired tiles (launches with entry nodes; tests/retire_model.py): root-culled or empty S -- the
    # fill workgroups' tiles, the group slots of the compacted order whose wavefronts leave at once
    # (every tile retired), and the fill path's column runs per tile-row (one for a whole tile-row)
    retire = None
    if 2 <= F <= 56:
        import retire_model as R
        import tile_compact_model as C
        ret, rects = R.retired_tiles(pkg, cut, b12, root, W, H)
        info = pkg.kept_tiles(W, H, F, tpw, [list(r) for r in rects])
        retire = R.counts(ret, rects, W, H, info["source"], info["packed"], tpw, info["deal"])
        dead_root = C.culled_tiles(rects, W, H)
        for key, dead in (("fill_runs", ret), ("fill_runs_root_cull_only", dead_root)):
            retire[key] = sum(1 if dead[f, by].all() else len(R.row_runs(dead[f, by])) for f in range(F) for by in range(ty))
        retire["idle_wavefront_share"] = round(retire["flagged_groups"] / max(1, retire["kept_groups"]), 4)
        retire["groups_for_perfect_packing"] = (retire["live_tiles"] + tpw - 1) // tpw
    print(json.dumps({"config": name, "frames": F, "views": views, "tiles": tiles, "culled_tiles": culled, "retire": retire,
                      "tiles_per_wave": tpw, "wave_groups": groups, "all_culled_groups": empty,
                      "all_culled_group_share": None if empty is None else round(empty / groups, 4),
                      "culled_tile_share": round(culled / tiles, 4), "culled_pixel_share": round(px_culled / (F * W * H), 4),
                      "tile_path_store_instr_all_tiles": 4 * tiles, "tile_path_store_instr_culled_tiles": 4 * culled,
                      "fill_path_store_instr": fill_instr,
                      "cut_nodes": cut.n, "entry_ok": cut.entry_ok, "kept_tiles_empty_S": empty_s,
                      "entry_depth_histogram": dict(sorted(depth_hist.items()))}))


if __name__ == "__main__":
    main()
