"""A pure-Python restatement of the retired tiles of a batch launch with entry nodes
(render_hip.hip: ceres_cull_rows' live mask, fill_retired_runs, ceres_order_compact's group flags,
the tile path of ceres_fused).  A tile is retired when it is root-culled (cull_fill_model's
tile_misses_root) or no cut rectangle reaches it (entry_tiles == ENTRY_EMPTY); retired tiles are
written by the fill path as maximal runs of tile columns per tile-row, every other tile by the tile
path, and a group slot of the compacted order is flagged when no tile of its group is live.
Nothing here is read by the product."""
import numpy as np

import cull_fill_model as M
import tile_compact_model as C


TWO_DIST = 1.5                                                       # tile_compact_model.look's distance for the two-object scene


def two_patches(pkg, n=12, gap=5.0, scale=1.0):
    """Two small proc_mesh patches far apart on x: (mesh, bvh)."""
    a = pkg.proc_mesh(n, arith=pkg.ARITH_FMA)
    ta, tb = a.tri.copy(), a.tri.copy()
    for t, dx in ((ta, -gap / 2), (tb, gap / 2)):
        t[:, 0:3] *= scale
        t[:, 3:9] *= scale
        t[:, 0] += dx
    mesh = pkg.Mesh(np.concatenate([ta, tb]), np.concatenate([a.norm, a.norm]))
    return mesh, pkg.build_bvh(mesh, arith=pkg.ARITH_FMA)


def between_rows(retired_f):
    """The tile-rows with a retired run strictly between live tiles."""
    return [by for by in range(retired_f.shape[0])
            if any(not retired_f[by, :x0].all() and not retired_f[by, x1:].all() for x0, x1 in row_runs(retired_f[by]))]


def host_cut(pkg, mesh, bvh):
    pairs, _, rlc = pkg.entry_relayout(mesh, bvh)
    return pkg.entry_cut(pairs, rlc, bvh.nodes[0, :6].copy().view(np.float32))


def retired_tiles(pkg, cut, b12, root, W, H):
    """(retired[f, tile row, tile column], the frames' cull rectangles): root-culled, or S empty."""
    rects = [M.cull_rect(b, root, W, H) for b in b12]
    out = C.culled_tiles(rects, W, H)
    for f, b in enumerate(b12):
        entry = pkg.entry_tiles(cut, pkg.entry_rects(cut, np.asarray(b, np.float32), W, H), W, H)
        out[f] |= entry == pkg.ENTRY_EMPTY
    return out, rects


def row_runs(dead):
    """Maximal runs [first, end) of True in a 1-D bool array."""
    d = np.concatenate([[False], np.asarray(dead, bool), [False]]).astype(np.int8)
    e = np.diff(d)
    return list(zip(np.flatnonzero(e == 1), np.flatnonzero(e == -1)))


def fill_runs(retired_f, W, H):
    """fill_retired_runs for every tile-row of one whole frame: (float runs, RGB8 runs), each (first
    element, elements) relative to the frame's base -- the whole rows in one run when the tile-row
    has no live tile, else every maximal run of retired tile columns, row by row."""
    fl, rg = [], []
    for by in range((H + 7) // 8):
        n = min(8, H - 8 * by)
        if retired_f[by].all():
            lo, hi = 8 * by, 8 * by + n - 1
            fl.append((3 * lo * W, 3 * n * W))
            rg.append((3 * (H - 1 - hi) * W, 3 * n * W))
            continue
        for x0, x1 in row_runs(retired_f[by]):
            a, b = 8 * int(x0), min(8 * int(x1), W)
            for k in range(n):
                row = 8 * by + k
                fl.append((3 * (row * W + a), 3 * (b - a)))
                rg.append((3 * ((H - 1 - row) * W + a), 3 * (b - a)))
    return fl, rg


def check_partition(retired_f, W, H, px_addr=0, rgb_addr=0):
    """Every pixel of the frame is written exactly once -- by the tile path (live tiles) or by a fill
    run -- in the float framebuffer and in the RGB8 body (rows flipped), byte for byte."""
    live_px = np.repeat(np.repeat(~retired_f, 8, 0), 8, 1)[:H, :W].astype(np.int32)
    fl, rg = fill_runs(retired_f, W, H)
    for runs, tile_cnt, size, addr in ((fl, live_px, 4, px_addr), (rg, live_px[::-1], 1, rgb_addr)):
        flat = np.zeros(3 * H * W * size, np.int32)                  # per byte
        for s, n in runs:
            assert n > 0 and 0 <= s and s + n <= 3 * H * W and s % 3 == 0 and n % 3 == 0, (s, n)
            M.zero_run_pieces(addr + s * size, n, size)
            flat[s * size:(s + n) * size] += 1
        total = flat.reshape(H, W, 3 * size) + tile_cnt[:, :, None]
        assert (total == 1).all(), ("float framebuffer" if size == 4 else "RGB8 body", W, H)
    return len(fl)


def group_flags(source, packed, tpw, rects, retired, W, H, deal):
    """(flag per group slot of the compacted order, kept groups): the order keeps the groups with a
    tile that is not root-culled (tile_compact_model); a slot is flagged when every tile of its
    group is retired."""
    f, by, bx = C.decode(source, packed, W, H)
    dead = retired[f, by, bx]
    pad = -len(dead) % tpw
    all_dead = np.concatenate([dead, np.ones(pad, bool)]).reshape(-1, tpw).all(axis=1)
    keep = C.kept_groups(source, packed, tpw, rects, W, H)
    idx, tiles = C.compact(np.arange(len(source), dtype=np.uint32), keep, tpw, deal)
    n = int(keep.sum())
    slots = idx[:n * tpw].reshape(-1, tpw)[:, 0].astype(np.int64) // tpw   # the source group of every slot
    assert np.array_equal(np.sort(slots), np.flatnonzero(keep))
    return all_dead[slots].astype(np.uint8), keep


def counts(retired, rects, W, H, source, packed, tpw, deal):
    """What tools/cull_share.py prints of a launch."""
    culled = C.culled_tiles(rects, W, H)
    flags, keep = group_flags(source, packed, tpw, rects, retired, W, H, deal)
    return {"tiles": int(retired.size), "root_culled_tiles": int(culled.sum()),
            "empty_S_tiles": int((retired & ~culled).sum()), "retired_tiles": int(retired.sum()),
            "live_tiles": int((~retired).sum()), "kept_groups": int(keep.sum()), "flagged_groups": int(flags.sum()),
            "working_groups": int(keep.sum() - flags.sum())}
