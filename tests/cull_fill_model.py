"""A pure-Python restatement of the background cull's two writers (render_hip.hip): the tile path
(a wavefront stores its tile unless tile_misses_root holds) and the fill path (fill_culled_rows:
whole rows, or the column runs beside the rectangle, per tile-row of 8 local rows), plus the
host's rectangle (cull_rect) -- for the partition check that runs without a GPU and for choosing
the cameras of tests/test_gpu_cull_fill.py.  Nothing here is read by the product."""
import math
from collections import namedtuple

import numpy as np

Rect = namedtuple("Rect", "i0 i1 j0 j1")
Tiling = namedtuple("Tiling", "row_block rank world bands")
KEEP = Rect(0, 0xffff, 0, 0xffff)
EMPTY = Rect(1, 0, 1, 0)


def whole(H):
    return Tiling(H, 0, 1, 0)


def local_rows(H, t):
    """ceres_tiling_local_rows: bands own row_block rows; row blocks are dealt round-robin."""
    if t.world == 1:
        return H
    if t.bands:
        return t.row_block
    nb = (H + t.row_block - 1) // t.row_block
    return sum(min(H, (b + 1) * t.row_block) - b * t.row_block for b in range(t.rank, nb, t.world))


def global_row(lr, f, t):
    if t.world == 1:
        return lr
    if t.bands:
        return ((t.rank + f) % t.world) * t.row_block + lr
    return ((lr // t.row_block) * t.world + t.rank) * t.row_block + lr % t.row_block


def root_box(mesh_tri):
    """The root node's bounds {x0, x1, y0, y1, z0, z1}: the triangles' vertices p0, p0 - e1, p0 + e2."""
    t = np.asarray(mesh_tri, np.float32).reshape(-1, 12)
    v = np.concatenate([t[:, 0:3], t[:, 0:3] - t[:, 3:6], t[:, 0:3] + t[:, 6:9]])
    lo, hi = v.min(0), v.max(0)
    return [float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2])]


def cull_rect(basis12, root, W, H):
    """cull_rect (render_hip.hip), line by line in double."""
    if W > 0xffff or H > 0xffff:
        return KEEP
    b = np.asarray(basis12, np.float32).astype(np.float64)
    e, d, iu, iv = b[0:3], b[3:6], b[6:9], b[9:12]
    sc = max(float(np.abs(e).max()), max(abs(float(x)) for x in root))
    pad = 1e-4 * sc
    c0, c1, c2 = np.cross(iv, d), np.cross(d, iu), np.cross(iu, iv)
    det = float(iu @ c0)
    u0 = v0 = math.inf
    u1 = v1 = -math.inf
    with np.errstate(all="ignore"):
        for k in range(8):
            X = np.array([root[1] + pad if k & 1 else root[0] - pad, root[3] + pad if k & 2 else root[2] - pad,
                          root[5] + pad if k & 4 else root[4] - pad])
            r = X - e
            pw, qw, ww = float(r @ c0), float(r @ c1), float(r @ c2)
            if not (np.float64(ww) / np.float64(det) > 0.01 * math.sqrt(float(r @ r))):
                return KEEP
            u0, u1 = min(u0, pw / ww), max(u1, pw / ww)
            v0, v1 = min(v0, qw / ww), max(v1, qw / ww)
    m = 2e-3 * (1 + max(abs(u0), abs(u1), abs(v0), abs(v1)))

    def lo(x, n):
        return 0 if x <= 0 else n if x >= n else int(math.floor(x))
    a0, a1 = (u0 - m + 1) * W / 2 - 0.5 - 1, (u1 + m + 1) * W / 2 - 0.5 + 1
    b0, b1 = (v0 - m + 1) * H / 2 - 0.5 - 1, (v1 + m + 1) * H / 2 - 0.5 + 1
    if any(x != x for x in (a0, a1, b0, b1)):
        return KEEP
    if a1 < 0 or b1 < 0:
        return EMPTY
    return Rect(lo(a0, W), int(min(math.ceil(a1), 0xffff)), lo(b0, H), int(min(math.ceil(b1), 0xffff)))


# ---- the kernels' decision (cull_cols_hit, row_exists, tile_rows_hit, tile_misses_root)
def cols_hit(r, W, bx):
    a = 8 * bx
    b = min(a + 7, W - 1)
    return max(a, r.i0) <= min(b, r.i1)


def row_exists(lr, f, rows, H, t):
    return lr < rows and (not (t.bands and t.world > 1) or global_row(lr, f, t) < H)


def rows_hit(by, f, r, rows, H, t):
    return any(row_exists(lr, f, rows, H, t) and r.j0 <= global_row(lr, f, t) <= r.j1 for lr in range(8 * by, 8 * by + 8))


def tile_misses_root(r, W, bx, hit):
    return not (hit and cols_hit(r, W, bx))


def tile_path(r, W, H, t, f=0, cull=True):
    """Times the tile path stores each (local row, column) of frame f."""
    rows = local_rows(H, t)
    n = np.zeros((rows, W), np.int32)
    for by in range((rows + 7) // 8):
        hit = rows_hit(by, f, r, rows, H, t)
        for bx in range((W + 7) // 8):
            if cull and tile_misses_root(r, W, bx, hit):
                continue
            for lr in range(8 * by, min(8 * by + 8, rows)):
                if row_exists(lr, f, rows, H, t):
                    n[lr, 8 * bx:min(8 * bx + 8, W)] += 1
    return n


def fill_runs(r, W, H, t, f=0):
    """fill_culled_rows for every tile-row of frame f: (float runs, RGB8 runs), each (first element,
    elements) relative to the frame's base, elements = floats resp. bytes."""
    rows = local_rows(H, t)
    fl, rg = [], []
    for by in range((rows + 7) // 8):
        n = sum(1 for k in range(8) if row_exists(8 * by + k, f, rows, H, t))
        assert all(row_exists(8 * by + k, f, rows, H, t) for k in range(n)), "the existing rows are a prefix"
        if not n:
            continue
        hit = rows_hit(by, f, r, rows, H, t)
        kept = [bx for bx in range((W + 7) // 8) if not tile_misses_root(r, W, bx, hit)]
        if not kept:
            lo, hi = 8 * by, 8 * by + n - 1
            fl.append((3 * lo * W, 3 * n * W))
            rg.append((3 * (rows - 1 - hi) * W, 3 * n * W))
            continue
        assert kept == list(range(kept[0], kept[-1] + 1)), "the kept tile columns are contiguous"
        a, b = 8 * kept[0], min(8 * kept[-1] + 8, W)
        for k in range(n):
            row = 8 * by + k
            for base, out in ((3 * row * W, fl), (3 * (rows - 1 - row) * W, rg)):
                out.append((base, 3 * a))
                out.append((base + 3 * b, 3 * (W - b)))
    return [x for x in fl if x[1]], [x for x in rg if x[1]]


def zero_run_pieces(addr, n, size):
    """zero_run: (head elements, 16-B vectors, tail elements) for n elements of `size` bytes at byte
    address addr; asserts the vectors are aligned and the pieces add up."""
    mis = addr & 15
    head = min(n, (16 - mis) // size if mis else 0)
    rest = n - head
    nv = rest * size // 16
    tail = rest - nv * (16 // size)
    assert nv == 0 or (addr + head * size) % 16 == 0
    assert head * size < 16 and tail * size < 16 and head * size + 16 * nv + tail * size == n * size
    return head, nv, tail


def launch_culls_a_tile(r, W, H, t, f=0):
    rows = local_rows(H, t)
    tiles_x = (W + 7) // 8
    for by in range((rows + 7) // 8):
        if not any(row_exists(lr, f, rows, H, t) for lr in range(8 * by, 8 * by + 8)):
            continue
        hit = rows_hit(by, f, r, rows, H, t)
        if any(tile_misses_root(r, W, bx, hit) for bx in range(tiles_x)):
            return True
    return False


def check_partition(r, W, H, t, f=0, px_addr=0, rgb_addr=0):
    """Every existing pixel of frame f is written exactly once, by the tile path or by a fill run,
    in both buffers; rows that do not exist (a band past the frame) are written by neither."""
    rows = local_rows(H, t)
    cull = launch_culls_a_tile(r, W, H, t, f)
    n_px = tile_path(r, W, H, t, f, cull)
    n_rgb = n_px[::-1].copy()                                         # RGB8 rows are stored flipped
    if cull:
        fl, rg = fill_runs(r, W, H, t, f)
        for runs, cnt, size, addr in ((fl, n_px, 4, px_addr), (rg, n_rgb, 1, rgb_addr)):
            flat = np.zeros(3 * rows * W, np.int32)
            for s, n in runs:
                assert 0 <= s and s + n <= flat.size and s % 3 == 0 and n % 3 == 0, (s, n)
                zero_run_pieces(addr + s * size, n, size)
                flat[s:s + n] += 1
            per_px = flat.reshape(rows, W, 3)
            assert (per_px == per_px[:, :, :1]).all()
            cnt += per_px[:, :, 0]
    want = np.array([[1 if row_exists(lr, f, rows, H, t) else 0] * W for lr in range(rows)], np.int32).reshape(rows, W)
    assert np.array_equal(n_px, want), ("float framebuffer", r, W, H, t, f)
    assert np.array_equal(n_rgb, want[::-1]), ("RGB8 body", r, W, H, t, f)
    return cull


# ---- the fused kernel's grid (launch_chunk / ceres_fused): tile groups and fill groups
def fused_grid(tile_groups, fill_tasks, spread=True):
    """(grid size, fill_stride, fill_magic) as launch_chunk sets them."""
    if spread and fill_tasks:
        nto, nfo = (tile_groups + 7) // 8, (fill_tasks + 7) // 8
        stride = (nto + nfo) // nfo
        if stride >= 2 and (nto + nfo) * stride < 1 << 32:
            return (nto + nfo) * 8, stride, ((1 << 32) + stride - 1) // stride
    return tile_groups + fill_tasks, 0, 0


def fused_block(b, grid, tile_groups, stride, magic):
    """What workgroup b of the grid is: ("fill", task), ("tile", group) or None (padding)."""
    if stride:
        octet, x, nfo = b >> 3, b & 7, (grid >> 3) - (tile_groups + 7) // 8
        q = (octet * magic) >> 32
        r = octet - q * stride
        if r == stride - 1 and q < nfo:
            return "fill", q * 8 + x
        g = (octet - min(q, nfo)) * 8 + x
        return ("tile", g) if g < tile_groups else None
    return ("fill", b - tile_groups) if b >= tile_groups else ("tile", b)
