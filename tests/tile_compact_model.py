"""A pure-Python restatement of the batch launches' tile-order compaction (render_hip.hip:
count_kept_tiles on the host, ceres_cull_rows / ceres_order_count / ceres_order_compact on the
device): which wavefront groups of the order survive -- decided tile by tile with
cull_fill_model's restatement of the kernels' cull -- and where the XCD dealing puts them.  Also
the cameras the compaction tests share.  Nothing here is read by the product."""
import numpy as np

import cull_fill_model as M

X_BITS = Y_BITS = 13                                                 # pack_tile: frame << 26 | tile row << 13 | tile column


def decode(entries, packed, W, H):
    """(frame, tile row, tile column) of order entries: pack_tile words or linear tile ids."""
    e = np.asarray(entries, np.int64)
    if packed:
        return e >> (X_BITS + Y_BITS), (e >> X_BITS) & ((1 << Y_BITS) - 1), e & ((1 << X_BITS) - 1)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    f, rem = e // (tx * ty), e % (tx * ty)
    return f, rem // tx, rem % tx


def culled_tiles(rects, W, H):
    """culled[f, tile row, tile column]: the kernels' tile_misses_root for every tile of whole frames."""
    tx, ty, t = (W + 7) // 8, (H + 7) // 8, M.whole(H)
    out = np.zeros((len(rects), ty, tx), bool)
    for f, r in enumerate(rects):
        for by in range(ty):
            hit = M.rows_hit(by, f, r, H, H, t)
            for bx in range(tx):
                out[f, by, bx] = M.tile_misses_root(r, W, bx, hit)
    return out


def kept_groups(source, packed, tpw, rects, W, H):
    """Per group of tpw consecutive source entries (the last may be short): a tile is not culled."""
    f, by, bx = decode(source, packed, W, H)
    live = ~culled_tiles(rects, W, H)[f, by, bx]
    pad = -len(live) % tpw
    return np.concatenate([live, np.zeros(pad, bool)]).reshape(-1, tpw).any(axis=1)


def compact(source, keep, tpw, deal):
    """(the compacted order zero-padded to a multiple of 8 entries, kept tiles): the kept groups in
    source order, whole; then, in the full runs of 8 chunks of `deal` groups, wavefront w of a run
    reads chunk w % 8, group w // 8 of it (ensure_tile_order's dealing, on the compacted curve)."""
    src = np.asarray(source, np.uint32)
    pad = -len(src) % tpw
    g = np.concatenate([src, np.zeros(pad, np.uint32)]).reshape(-1, tpw)[keep]
    tiles = len(g) * tpw - (pad if len(keep) and keep[-1] else 0)
    if deal:
        run = 8 * deal
        dealt = tiles // (run * tpw) * run
        w = np.arange(dealt)
        wl = w % run
        g = np.concatenate([g[w - wl + (wl % 8) * deal + wl // 8], g[dealt:]])
    flat = g.reshape(-1)
    padded = (tiles + 7) // 8 * 8
    return np.concatenate([flat, np.zeros(max(0, padded - len(flat)), np.uint32)])[:padded], tiles


# ---- cameras (on the bunny: root = cull_fill_model.root_box of its triangles)
def scene_frame(root):
    lo, hi = np.array(root[0::2]), np.array(root[1::2])
    return (lo + hi) / 2, float(np.linalg.norm(hi - lo))


def look(pkg, root, W, H, yaw=0.0, pitch=0.0, dist=2.0, fov=40.0, eye=None):
    """basis12 of a camera `dist` scene diagonals in front of the mesh, turned away from its centre
    by yaw / pitch degrees (or at `eye`)."""
    ctr, diag = scene_frame(root)
    eye = ctr + np.array([0.0, 0.0, -dist * diag]) if eye is None else np.asarray(eye, np.float64)
    y, p = np.radians(yaw), np.radians(pitch)
    d = np.array([np.sin(y) * np.cos(p), np.sin(p), np.cos(y) * np.cos(p)])
    cam = pkg.Camera(eye.astype(np.float32), d.astype(np.float32), (0.0, 1.0, 0.0), fov, arith=pkg.ARITH_FMA)
    return np.asarray(cam.basis(W, H), np.float32)


def find(pkg, root, W, H, pred):
    """The first camera of a yaw x pitch sweep, three scene diagonals away, whose rectangle satisfies pred."""
    for a in np.linspace(-12.0, 12.0, 49):
        for b in np.linspace(-8.0, 8.0, 17):
            v = look(pkg, root, W, H, yaw=float(a), pitch=float(b), dist=3.0)
            if pred(M.cull_rect(v, root, W, H)):
                return v
    raise AssertionError("no camera of the sweep gives the wanted rectangle")


def cameras(pkg, root, W, H):
    """The named views of the compaction tests: `odd` -- the mesh partly in view, its rectangle inside
    the frame and starting on an odd tile column and an odd tile row; `gone` -- the mesh off the
    frame (empty rectangle: every tile culled); `inside` -- the eye in the root box (nothing culled);
    `centre` -- the mesh in the middle."""
    ctr, _ = scene_frame(root)
    v = {"centre": look(pkg, root, W, H),
         "odd": find(pkg, root, W, H, lambda r: r.i0 // 8 % 2 == 1 and r.j0 // 8 % 2 == 1 and r.i1 < W - 8 and r.j1 < H - 8),
         "gone": look(pkg, root, W, H, yaw=60.0),
         "inside": look(pkg, root, W, H, eye=ctr)}
    if M.cull_rect(v["gone"], root, W, H) != M.EMPTY:
        v["gone"] = look(pkg, root, W, H, yaw=-60.0)
    assert M.cull_rect(v["gone"], root, W, H) == M.EMPTY and M.cull_rect(v["inside"], root, W, H) == M.KEEP
    return v


# the batches of the tests: (W, H, tiles per wave, the views of the frames)
BATCHES = [(136, 72, 4, ("odd", "gone", "centre")),
           (136, 72, 4, ("inside", "gone", "odd", "centre", "gone")),
           (1024, 1024, 2, ("odd", "gone")),
           (1160, 904, 2, ("inside", "odd")),
           (1024, 1024, 2, ("odd", "centre", "gone", "inside", "odd", "centre", "gone", "centre", "odd"))]
