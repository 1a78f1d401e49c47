"""Culled background tiles are written by the fill workgroups of the same launch, not by the
wavefronts that meet them in the tile order (render_hip.hip fill_culled_rows).

GPU cases: the bunny through a production scene and through a CERES_SCENE_STATS scene (which never
culls), the same call on both, into device buffers pre-filled with 0xA5 bytes and 64 guard bytes
behind them: every byte of both buffers and the ray / hit / primary / shadow counts must agree, so
a pixel no path wrote (it keeps the pattern), one written past its run (the guards, the rows of a
band past the frame) and a stale stash all show.  Small frames are also pinned to the oracle.
The band tiling has no stats instantiation: its reference is the stats scene rendering each frame's
band as the one row block of a row-block tiling, placed by the host.

Without a GPU: cull_fill_model restates both writers; every existing pixel must be written by
exactly one of them, for the shapes and tilings below and for random rectangles."""
import numpy as np
import pytest

import configs
import cull_fill_model as M

SIZES = [(1, 1), (8, 8), (37, 29), (333, 217), (640, 480)]
TILINGS = [(8, 1, 2), (8, 3, 8), (16, 1, 2), (16, 4, 8)]             # (row_block, rank, world)


# ------------------------------------------------------------------ host-side partition check
def _rects(W, H, rng, n):
    out = [M.KEEP, M.EMPTY, M.Rect(0, W // 2, 0, H // 2), M.Rect(W // 3, 0xffff, H // 3, 0xffff), M.Rect(W, 0xffff, 0, 0xffff),
           M.Rect(8, 15, 8, 15), M.Rect(9, 14, 9, 14), M.Rect(W - 1, W - 1, H - 1, H - 1), M.Rect(0, 0, 0, 0)]
    for _ in range(n):
        i = sorted(int(x) for x in rng.integers(0, W + 9, 2))
        j = sorted(int(x) for x in rng.integers(0, H + 9, 2))
        out.append(M.Rect(i[0], i[1], j[0], j[1]))
    return out


@pytest.mark.parametrize("W,H", SIZES + [(1920, 1080)])
def test_tile_path_and_fill_path_partition_the_frame(W, H):
    rng = np.random.default_rng(W * 7 + H)
    big = W * H > 100000
    culls = 0
    for k, r in enumerate(_rects(W, H, rng, 3 if big else 40)):
        culls += M.check_partition(r, W, H, M.whole(H), px_addr=4 * (k % 4), rgb_addr=k % 16)
    assert not M.launch_culls_a_tile(M.KEEP, W, H, M.whole(H))
    assert culls or (W, H) == (1, 1)


@pytest.mark.parametrize("rb,rank,world", TILINGS)
def test_partition_under_row_block_tilings(rb, rank, world):
    W, H = 333, 217
    rng = np.random.default_rng(rb * 100 + world)
    for k, r in enumerate(_rects(W, H, rng, 25)):
        M.check_partition(r, W, H, M.Tiling(rb, rank, world, 0), px_addr=4 * (k % 4), rgb_addr=k % 16)


def test_partition_under_bands():
    W, H = 100, 61                                                   # 4 bands of 16 rows: the last one has 13
    rng = np.random.default_rng(5)
    for k, r in enumerate(_rects(W, H, rng, 25)):
        for rank in range(4):
            for f in (0, 1, 30):
                M.check_partition(r, W, H, M.Tiling(16, rank, 4, 1), f=f, px_addr=4 * (k % 4), rgb_addr=k % 16)


@pytest.mark.parametrize("tile_groups,fill_tasks", [(1, 1), (1, 9), (3, 28), (21, 84), (27, 28), (4800, 60), (259200, 2160),
                                                    (1048576, 8192), (32400, 135), (7, 1), (8, 8), (9, 8), (1000, 999)])
def test_every_tile_group_and_fill_task_has_one_workgroup(tile_groups, fill_tasks):
    """The fused kernel's grid with fill groups spread in octets: each tile group and each fill
    task is exactly one workgroup, a tile group keeps its index mod 8 (its XCD), fill tasks past
    the launch's count are the only extras, and the multiply-high division is exact."""
    grid, stride, magic = M.fused_grid(tile_groups, fill_tasks)
    tiles, fills = [], []
    for b in range(grid):
        if stride:
            assert ((b >> 3) * magic) >> 32 == (b >> 3) // stride
        w = M.fused_block(b, grid, tile_groups, stride, magic)
        if w and w[0] == "tile":
            assert w[1] % 8 == b % 8 or not stride
            tiles.append(w[1])
        elif w:
            fills.append(w[1])
    assert tiles == list(range(tile_groups))
    assert sorted(fills) == list(range(len(fills))) and fill_tasks <= len(fills) < fill_tasks + 8


# ------------------------------------------------------------------ GPU cases
class _Env:
    pass


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    e = _Env()
    e.pkg = pkg
    e.cfg = configs.CONFIGS["bunny_1080"]
    e.mesh, e.bvh, _ = pkg.prepare(e.cfg, arith=pkg.ARITH_FMA)
    e.prod, e.ref = pkg.Scene(e.mesh, e.bvh), pkg.Scene(e.mesh, e.bvh, stats=True)
    e.root = M.root_box(e.mesh.tri)
    lo, hi = np.array(e.root[0::2]), np.array(e.root[1::2])
    e.ctr, e.diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    e.sun = np.asarray(e.cfg["sun"], np.float32)
    e.full = pkg.MODE_FULL | pkg.MODE_FMA
    e.primary = pkg.MODE_PRIMARY | pkg.MODE_FMA
    e.oracle = None
    yield e
    e.prod.close()
    e.ref.close()


def _look(e, W, H, yaw=0.0, pitch=0.0, dist=2.0, fov=40.0, eye=None):
    """basis12 of a camera `dist` scene diagonals in front of the bunny, turned away from its
    centre by yaw / pitch degrees."""
    eye = e.ctr + np.array([0.0, 0.0, -dist * e.diag]) if eye is None else np.asarray(eye, np.float64)
    y, p = np.radians(yaw), np.radians(pitch)
    d = np.array([np.sin(y) * np.cos(p), np.sin(p), np.cos(y) * np.cos(p)])
    cam = e.pkg.Camera(eye.astype(np.float32), d.astype(np.float32), (0.0, 1.0, 0.0), fov, arith=e.pkg.ARITH_FMA)
    return cam.basis(W, H)


def _find(e, W, H, pred, axis="yaw"):
    """The first camera of a sweep whose rectangle (cull_fill_model.cull_rect) satisfies pred."""
    for a in np.linspace(-30.0, 30.0, 241):
        b = _look(e, W, H, **{axis: float(a)})
        r = M.cull_rect(b, e.root, W, H)
        if pred(r):
            return b, r
    raise AssertionError("no camera of the sweep gives the wanted rectangle")


def _call(e, scene, b12, W, H, mode, tiling, rows, want_px, want_rgb, px_off, rgb_off):
    import torch
    F = len(b12)
    n = 3 * F * rows * W
    px = torch.full((px_off + 4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.full((rgb_off + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert px.data_ptr() % 16 == 0 and rgb.data_ptr() % 16 == 0
    s3 = np.repeat(e.sun[None], F, 0)
    scene.render_batch_device(b12, s3, W, H, mode=mode, tiling=tiling, d_pixels=px.data_ptr() + px_off if want_px else 0,
                              d_rgb8=rgb.data_ptr() + rgb_off if want_rgb else 0, d_counters=cnt.data_ptr())
    torch.cuda.synchronize()
    return px.cpu().numpy(), rgb.cpu().numpy(), [int(x) for x in cnt.cpu().numpy()[:4]]


def _same(e, b12, W, H, mode=None, tiling=None, want_px=True, want_rgb=True, px_off=0, rgb_off=0):
    """The same call on the production and the stats scene: every byte and count equal; returns
    the production scene's (float bytes, RGB8 bytes, counts)."""
    b12 = np.asarray(b12, np.float32).reshape(-1, 12)
    mode = e.full if mode is None else mode
    t = e.pkg.Tiling(*tiling, 0) if tiling else None
    rows = e.pkg.local_rows(H, t) if t else H
    a = _call(e, e.prod, b12, W, H, mode, t, rows, want_px, want_rgb, px_off, rgb_off)
    b = _call(e, e.ref, b12, W, H, mode, t, rows, want_px, want_rgb, px_off, rgb_off)
    assert a[2] == b[2]
    assert np.array_equal(a[0], b[0]), "float framebuffer (or its surroundings) differs"
    assert np.array_equal(a[1], b[1]), "RGB8 body (or its surroundings) differs"
    if not want_px:
        assert (a[0] == 0xA5).all()
    if not want_rgb:
        assert (a[1] == 0xA5).all()
    return a


def _oracle(e, b12, W, H, got, primary=False):
    import oracle
    if e.oracle is None:
        e.oracle = oracle.prepare(e.cfg, contract=True)
    cfg = dict(e.cfg, W=W, H=H, mode="primary" if primary else "full")
    ref = oracle.render(e.oracle, cfg, basis=b12[3:], eye=b12[:3], sun=e.sun)
    n = 3 * W * H
    assert np.array_equal(got[0][:4 * n].view(np.uint32), ref["pixels"].view(np.uint32))
    assert np.array_equal(got[1][:n], ref["ppm"])
    assert got[2][:2] == [ref["rays"], ref["hits"]]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_single_frames(env, W, H):
    """The one-frame (stealing) kernel and the primary-only kernel at every size; the rectangle
    lies inside the frame where the frame is large enough, so tiles on every side are culled."""
    e = env
    for b in (_look(e, W, H), _look(e, W, H, yaw=14.0, pitch=9.0)):  # centred; towards a corner
        if W >= 333:
            assert M.launch_culls_a_tile(M.cull_rect(b, e.root, W, H), W, H, M.whole(H))
        got = _same(e, b, W, H)
        gp = _same(e, b, W, H, mode=e.primary)
        if W * H <= 333 * 217:
            _oracle(e, b, W, H, got)
            _oracle(e, b, W, H, gp, primary=True)


@pytest.mark.gpu
def test_pair_kernel_with_odd_aligned_rectangles(env):
    """A 2-frame 1080p batch (2 tiles per wave, PairStash).  Frame 0: the rectangle starts in an odd
    tile column, so an even tile is culled and its odd partner stores alone; frame 1: it ends in an
    even tile column, so a stashed even tile's odd partner is culled."""
    e = env
    W, H = 1920, 1080
    b0, r0 = _find(e, W, H, lambda r: r.i0 // 8 % 2 == 1 and r.i1 < W - 16)
    b1, r1 = _find(e, W, H, lambda r: r.i1 // 8 % 2 == 0 and r.i0 > 16 and r.i1 < W - 16)
    assert r0.i0 > 8 and r1 != r0
    _same(e, [b0, b1], W, H)


@pytest.mark.gpu
def test_four_tile_kernel_batch_of_different_rectangles(env):
    """A 3-frame 640x480 batch (4 tiles per wave): a rectangle inside the frame, one clipped at
    the left edge, one with odd-aligned first column."""
    e = env
    W, H = 640, 480
    b0 = _look(e, W, H)
    b1, r1 = _find(e, W, H, lambda r: r.i0 == 0 and 8 < r.i1 < W - 16)
    b2, r2 = _find(e, W, H, lambda r: r.i0 // 8 % 2 == 1 and r.i1 < W - 16)
    assert len({M.cull_rect(b0, e.root, W, H), r1, r2}) == 3
    _same(e, [b0, b1, b2], W, H)


@pytest.mark.gpu
def test_narrow_frames_keep_the_fill_groups_last(env):
    """A 3-frame batch of 8x217 frames: more fill octets than tile octets, so the grid is not
    interleaved (cull_fill_model.fused_grid: stride 0) and the fill groups are its last ones."""
    e = env
    W, H = 8, 217
    assert M.fused_grid((3 * 28 + 3) // 4, 3 * 28)[1] == 0
    b = [_look(e, W, H, fov=70.0), _look(e, W, H, fov=70.0, pitch=12.0), _look(e, W, H, fov=70.0, pitch=-15.0)]
    assert all(M.launch_culls_a_tile(M.cull_rect(x, e.root, W, H), W, H, M.whole(H)) for x in b)
    _same(e, b, W, H)


@pytest.mark.gpu
def test_empty_and_whole_rectangles(env):
    """The mesh off the left edge (empty rectangle) and off the right edge: the whole frame is
    filled; the eye inside the root box: nothing is culled and the launch has no fill groups; a
    rectangle clipped at the bottom edge."""
    e = env
    W, H = 333, 217
    left = _look(e, W, H, yaw=60.0)
    right = _look(e, W, H, yaw=-60.0)
    rl, rr = M.cull_rect(left, e.root, W, H), M.cull_rect(right, e.root, W, H)
    assert M.EMPTY in (rl, rr)
    for r in (rl, rr):
        assert not any(M.cols_hit(r, W, bx) for bx in range((W + 7) // 8))
    inside = _look(e, W, H, eye=e.ctr)
    assert M.cull_rect(inside, e.root, W, H) == M.KEEP and not M.launch_culls_a_tile(M.KEEP, W, H, M.whole(H))
    edge, re_ = _find(e, W, H, lambda r: r.j0 == 0 and 8 < r.j1 < H - 16, axis="pitch")
    for b in (left, right, inside, edge):
        got = _same(e, b, W, H)
        _oracle(e, b, W, H, got)
    got = _same(e, [left, inside, edge, right], W, H)                # and as one batch
    assert got[2][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("want_px,want_rgb,px_off,rgb_off", [(True, False, 0, 0), (False, True, 0, 0), (True, True, 0, 0),
                                                             (True, True, 4, 1), (True, True, 12, 15)])
def test_buffers_absent_and_misaligned(env, want_px, want_rgb, px_off, rgb_off):
    e = env
    W, H = 333, 217
    b = [_look(e, W, H), _look(e, W, H, yaw=6.0, pitch=-4.0)]
    _same(e, b, W, H, want_px=want_px, want_rgb=want_rgb, px_off=px_off, rgb_off=rgb_off)
    _same(e, b[:1], W, H, want_px=want_px, want_rgb=want_rgb, px_off=px_off, rgb_off=rgb_off)
    _same(e, b[:1], W, H, mode=e.primary, want_px=want_px, want_rgb=want_rgb, px_off=px_off, rgb_off=rgb_off)


@pytest.mark.gpu
@pytest.mark.parametrize("rb,rank,world", TILINGS)
def test_row_block_tilings(env, rb, rank, world):
    e = env
    W, H = 333, 217
    b = [_look(e, W, H), _look(e, W, H, yaw=5.0, pitch=8.0)]
    _same(e, b, W, H, tiling=(rb, rank, world))
    _same(e, b[:1], W, H, tiling=(rb, rank, world))
    _same(e, b[:1], W, H, mode=e.primary, tiling=(rb, rank, world))


@pytest.mark.gpu
def test_bands_with_a_second_launch(env):
    """60 frames of 100x61 in 4 bands of 16 rows (the last band has 13): two launches of 30 frames,
    the second with f0 = 30, so its frames' bands start at (rank + 30) mod 4."""
    import torch
    e = env
    pkg = e.pkg
    W, H, rb, world, rank, F = 100, 61, 16, 4, 1, 60
    views = [_look(e, W, H), _look(e, W, H, yaw=4.0, pitch=3.0), _look(e, W, H, yaw=-5.0, pitch=-6.0)]
    b12 = np.stack([views[f % 3] for f in range(F)]).astype(np.float32)
    n = 3 * F * rb * W
    got = _call(e, e.prod, b12, W, H, e.full, pkg.Tiling(rb, rank, world, 1), rb, True, True, 4, 1)
    want_px = np.full(4 + 4 * n + 64, 0xA5, np.uint8)
    want_rgb = np.full(1 + n + 64, 0xA5, np.uint8)
    wp = want_px[4:4 + 4 * n].view(np.float32).reshape(F, rb, W, 3)
    wr = want_rgb[1:1 + n].reshape(F, rb, W, 3)
    counts = [0, 0, 0, 0]
    cache = {}
    for f in range(F):
        band = (rank + f) % world
        if (f % 3, band) not in cache:
            rows = pkg.local_rows(H, pkg.Tiling(rb, band, world, 0))
            cache[f % 3, band] = _call(e, e.ref, b12[f:f + 1], W, H, e.full, pkg.Tiling(rb, band, world, 0), rows, True, True,
                                       0, 0) + (rows,)
        px, rgb, c, rows = cache[f % 3, band]
        wp[f, :rows] = px[:12 * rows * W].view(np.float32).reshape(rows, W, 3)
        wr[f, rb - rows:] = rgb[:3 * rows * W].reshape(rows, W, 3)    # a band's RGB8 rows: flipped within row_block rows
        counts = [x + y for x, y in zip(counts, c)]
    assert got[2] == counts
    assert np.array_equal(got[0], want_px)
    assert np.array_equal(got[1], want_rgb)
    torch.cuda.synchronize()
