"""The host's count of the tiles a compacted batch order keeps (count_kept_tiles, through
ceres_debug_kept_tiles: no GPU) against tile_compact_model's plain restatement -- the kernels' cull
decided for every tile, the groups formed on the returned source order -- for the views of the GPU
compaction tests and for random rectangles.  The launch sizes its grid by this count, and the
device raises the launch's error word when its own count differs (tests/test_gpu_tile_compact.py)."""
import numpy as np
import pytest

import configs
import cull_fill_model as M
import tile_compact_model as C


@pytest.fixture(scope="module")
def root(pkg):
    mesh, _, _ = pkg.prepare(configs.CONFIGS["bunny_1080"], arith=pkg.ARITH_FMA)
    return M.root_box(mesh.tri)


def _check(pkg, W, H, tpw, rects, count=None):
    got = pkg.kept_tiles(W, H, len(rects), tpw, [list(r) for r in rects])
    n = ((W + 7) // 8) * ((H + 7) // 8) * len(rects)
    # how the host counts: the subset-box sums where every frame holds the same whole groups of at
    # most 4 tiles, else a walk over an order of at most 65,536 entries
    per_frame = n // len(rects)
    assert got["count"] == (count or ("boxes" if per_frame % tpw == 0 and tpw <= 4 and W * H >= 1 << 20 else "walk"))
    f, by, bx = C.decode(got["source"], got["packed"], W, H)
    ids = (f * ((H + 7) // 8) + by) * ((W + 7) // 8) + bx
    assert np.array_equal(np.sort(ids), np.arange(n)), "the source order holds every tile once"
    keep = C.kept_groups(got["source"], got["packed"], tpw, rects, W, H)
    _, tiles = C.compact(got["source"], keep, tpw, got["deal"])
    assert got["tiles"] == tiles, (W, H, tpw, rects)
    return keep


@pytest.mark.parametrize("W,H,tpw,views", C.BATCHES)
def test_host_count_for_the_test_views(pkg, root, W, H, tpw, views):
    cams = C.cameras(pkg, root, W, H)
    rects = [M.cull_rect(cams[v], root, W, H) for v in views]
    keep = _check(pkg, W, H, tpw, rects)
    assert keep.any() and not keep.all()
    assert (W * H >= 1 << 20) == (pkg.kept_tiles(W, H, len(rects), tpw, [list(r) for r in rects])["deal"] != 0)


@pytest.mark.parametrize("W,H,tpw,frames", [(136, 72, 4, 3), (333, 217, 4, 2), (1160, 904, 2, 2), (1030, 1020, 8, 3),
                                            (1024, 1024, 2, 3), (1040, 1024, 4, 2), (1920, 1080, 2, 2)])
def test_host_count_for_random_rectangles(pkg, W, H, tpw, frames):
    """10 batches of random rectangles per shape: shuffled orders (walked), the Morton curve with an odd
    tile count per frame (walked) and with whole groups per frame (subset boxes: 1024^2 pairs, 130 x 128
    tiles in fours -- the curve's jumps at the frame's edges give the groups many extents -- and the
    flagship's 240 x 135 tiles in pairs)."""
    rng = np.random.default_rng(W + 3 * H + frames)
    for k in range(10):
        rects = []
        for _ in range(frames):
            i = sorted(int(x) for x in rng.integers(0, W + 9, 2))
            j = sorted(int(x) for x in rng.integers(0, H + 9, 2))
            kind = (k + len(rects)) % 4                              # 0: keeps every tile, 1: culls every tile
            rects.append(M.KEEP if kind == 0 else M.EMPTY if kind == 1 else M.Rect(i[0], i[1], j[0], j[1]))
        _check(pkg, W, H, tpw, rects)


def test_all_kept_and_all_culled(pkg):
    W, H = 136, 72
    n = 17 * 9 * 2
    assert pkg.kept_tiles(W, H, 2, 4, [list(M.KEEP)] * 2)["tiles"] == n
    assert pkg.kept_tiles(W, H, 2, 4, [list(M.EMPTY)] * 2)["tiles"] == 0
    # 17 x 9 x 3 = 459 tiles: the last group of 4 holds 3; kept alone, it counts 3
    got = pkg.kept_tiles(W, H, 3, 4, [list(M.KEEP)] * 3)
    assert got["tiles"] == 459
    f, by, bx = C.decode(got["source"][-1:], got["packed"], W, H)
    only = [M.EMPTY] * 3
    only[int(f[0])] = M.Rect(8 * int(bx[0]), 8 * int(bx[0]), 8 * int(by[0]), 8 * int(by[0]))
    assert pkg.kept_tiles(W, H, 3, 4, [list(r) for r in only])["tiles"] == 3


def test_an_order_without_a_cheap_count_is_not_compacted(pkg):
    """5 frames of 145 x 113 tiles in pairs: an odd tile count per frame, so the frames' groups differ,
    and more than 65,536 entries to walk -- the host reports every tile, and launches keep the plain grid."""
    got = pkg.kept_tiles(1160, 904, 5, 2, [list(M.EMPTY)] * 5)
    assert got["count"] is None and got["tiles"] == 145 * 113 * 5
