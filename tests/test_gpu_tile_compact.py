"""Batch launches that cull read a compacted tile order: the wavefront groups whose tiles are all
culled are dropped on the device ahead of the kernel (render_hip.hip ceres_order_compact), and the
grid is sized by the host's count of the rest.

Image parity: every byte of the float framebuffer and of the RGB8 body (both pre-filled with 0xA5,
64 guard bytes behind them) and the ray / hit / primary / shadow counts of the batch launch equal
the same frames rendered one per launch on a CERES_SCENE_STATS scene, which never culls or
compacts; the launch's error word is 0.  The order: ceres_debug_compact_order returns what the
launch read, and it must be tile_compact_model's compaction of the source order -- exactly the
groups with a tile that is not culled, each once, dealt to the XCDs chunk by chunk -- with the
device's count equal to the host's.  Tilings with world > 1 keep the plain grid."""
import numpy as np
import pytest

import configs
import cull_fill_model as M
import tile_compact_model as C


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
    e.sun = np.asarray(e.cfg["sun"], np.float32)
    e.full = pkg.MODE_FULL | pkg.MODE_FMA
    e.cams, e.refs = {}, {}
    yield e
    e.prod.close()
    e.ref.close()


def _cams(e, W, H):
    if (W, H) not in e.cams:
        e.cams[W, H] = C.cameras(e.pkg, e.root, W, H)
    return e.cams[W, H]


def _call(e, scene, b12, W, H, tiling, rows):
    """One batch call into patterned buffers -> (float bytes, RGB8 bytes, guards ok, 8 counters)."""
    import torch
    F = len(b12)
    n = 3 * F * rows * W
    px = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    scene.render_batch_device(b12, np.repeat(e.sun[None], F, 0), W, H, mode=e.full, tiling=tiling, d_pixels=px.data_ptr(),
                              d_rgb8=rgb.data_ptr(), d_counters=cnt.data_ptr())
    torch.cuda.synchronize()
    px, rgb = px.cpu().numpy(), rgb.cpu().numpy()
    assert (px[4 * n:] == 0xA5).all() and (rgb[n:] == 0xA5).all(), "a store behind the buffers"
    return px[:4 * n].reshape(F, -1), rgb[:n].reshape(F, -1), [int(x) for x in cnt.cpu().numpy()]


def _ref(e, name, b, W, H, tiling_key, tiling, rows):
    """The stats scene's one-frame launch of a view: computed once, shared, never changed."""
    key = (name, W, H, tiling_key)
    if key not in e.refs:
        px, rgb, c = _call(e, e.ref, b[None], W, H, tiling, rows)
        px.setflags(write=False)
        rgb.setflags(write=False)
        e.refs[key] = (px[0], rgb[0], c[:4])
    return e.refs[key]


def _parity(e, W, H, views, tiling=None):
    """The batch on the production scene against the frames one per launch on the stats scene."""
    cams = _cams(e, W, H)
    b12 = np.stack([cams[v] for v in views])
    t = e.pkg.Tiling(*tiling, 0) if tiling else None
    rows = e.pkg.local_rows(H, t) if t else H
    px, rgb, c = _call(e, e.prod, b12, W, H, t, rows)
    assert c[6] == 0, "the launch's error word"
    want = [0, 0, 0, 0]
    for f, v in enumerate(views):
        rp, rr, rc = _ref(e, v, cams[v], W, H, tiling, t, rows)
        assert np.array_equal(px[f], rp), f"float framebuffer of frame {f} ({v}) differs"
        assert np.array_equal(rgb[f], rr), f"RGB8 body of frame {f} ({v}) differs"
        want = [x + y for x, y in zip(want, rc)]
    assert c[:4] == want
    return [M.cull_rect(cams[v], e.root, W, H) for v in views]


def _check_order(e, W, H, tpw, rects):
    """What the launch read is the model's compaction of its source order."""
    got = e.prod.compact_order()
    assert got is not None, "the launch took the plain grid"
    assert got["tpw"] == tpw
    packed = True                                                    # these batches fit pack_tile's fields
    f, by, bx = C.decode(got["source"], packed, W, H)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    assert np.array_equal(np.sort((f * ty + by) * tx + bx), np.arange(tx * ty * len(rects))), "the source order holds every tile once"
    keep = C.kept_groups(got["source"], packed, tpw, rects, W, H)
    want, tiles = C.compact(got["source"], keep, tpw, got["deal"])
    assert got["host_tiles"] == tiles and got["device_tiles"] == tiles and got["groups"] == int(keep.sum())
    assert np.array_equal(got["order"], want)
    # said again without the model's dealing: every kept group once, none else ...
    pad = -len(got["source"]) % tpw
    src_groups = np.concatenate([got["source"], np.zeros(pad, np.uint32)]).reshape(-1, tpw)
    index = {tuple(g): k for k, g in enumerate(src_groups)}
    assert len(index) == len(src_groups)
    pos = np.array([index[tuple(g)] for g in got["order"][:int(keep.sum()) * tpw].reshape(-1, tpw)])
    assert np.array_equal(np.sort(pos), np.flatnonzero(keep))
    # ... and in curve order within each XCD's chunks: in a full run of 8 x deal groups, XCD x's
    # wavefronts (slots x, x + 8, ...) walk `deal` consecutive kept groups; the rest keeps the order
    run = 8 * got["deal"]
    dealt = tiles // (run * tpw) * run if run else 0
    rank = np.searchsorted(np.flatnonzero(keep), pos)
    for r0 in range(0, dealt, run or 1):
        for x in range(8):
            assert np.array_equal(rank[r0 + x:r0 + run:8], r0 + x * got["deal"] + np.arange(got["deal"]))
    assert np.array_equal(rank[dealt:], np.arange(dealt, len(rank)))
    return dealt


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,tpw,views", C.BATCHES)
def test_batches_match_single_stats_frames_and_read_the_compacted_order(env, W, H, tpw, views):
    rects = _parity(env, W, H, views)
    dealt = _check_order(env, W, H, tpw, rects)
    got = env.prod.compact_order()
    assert (got["deal"] == 64) == (W * H >= 1 << 20), "frames of 1 Mpixel and more: the XCD-local curve, chunks of 128 tiles"
    if len(views) == 9:
        assert dealt > 0 and dealt * tpw < got["device_tiles"], "a full run of 8 chunks is dealt, and a tail is left"


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(136, 72), (1024, 1024)])
def test_a_batch_that_keeps_every_tile_takes_the_plain_grid(env, W, H):
    _parity(env, W, H, ("odd", "gone"))
    assert env.prod.compact_order() is not None
    _parity(env, W, H, ("inside", "inside", "inside"))
    assert env.prod.compact_order() is None


@pytest.mark.gpu
@pytest.mark.parametrize("rank", [0, 1])
def test_row_block_tilings_keep_the_plain_grid(env, rank):
    W, H = 136, 72
    _parity(env, W, H, ("odd", "gone", "centre"))
    assert env.prod.compact_order() is not None
    _parity(env, W, H, ("odd", "gone", "centre"), tiling=(16, rank, 2))
    assert env.prod.compact_order() is None


@pytest.mark.gpu
def test_band_tiling_keeps_the_plain_grid(env):
    """3 bands of 24 rows: frame f of the batch renders band (rank + f) mod 3; its reference is the
    stats scene rendering that band as the one row block of a row-block tiling."""
    e = env
    W, H, rb, world, rank = 136, 72, 24, 3, 1
    views = ("odd", "gone", "centre", "odd")
    cams = _cams(e, W, H)
    px, rgb, c = _call(e, e.prod, np.stack([cams[v] for v in views]), W, H, e.pkg.Tiling(rb, rank, world, 1), rb)
    assert c[6] == 0 and e.prod.compact_order() is None
    want = [0, 0, 0, 0]
    for f, v in enumerate(views):
        band = (rank + f) % world
        rp, rr, rc = _ref(e, v, cams[v], W, H, (rb, band, world), e.pkg.Tiling(rb, band, world, 0), rb)
        assert np.array_equal(px[f], rp) and np.array_equal(rgb[f], rr), f"frame {f} ({v}) differs"
        want = [x + y for x, y in zip(want, rc)]
    assert c[:4] == want


@pytest.mark.gpu
def test_a_call_of_two_launches(env):
    """60 frames of 136x72: two launches of 30 frames on one stream, each compacting for its own
    cameras into the stream's buffer."""
    e = env
    W, H = 136, 72
    names = ("odd", "gone", "centre", "inside", "gone")
    views = tuple(names[(f * f) % 5] for f in range(60))
    rects = _parity(e, W, H, views)
    _check_order(e, W, H, 4, rects[30:])                            # the second launch's order
