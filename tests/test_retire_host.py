"""Retired tiles on the host (no GPU): tests/retire_model.py restates which tiles of a launch with
entry nodes are retired (root-culled, or no cut rectangle reaches them: entry_tiles ==
ENTRY_EMPTY, through the library's own host entry points), the fill path's runs and the group
flags of the compacted order.

The fill runs and the live tiles partition every frame exactly, byte for byte, in the float
framebuffer and in the RGB8 body with its flipped rows; no pixel the oracle records a primary hit
for lies in a retired tile (the 20 views of test_entry_cut_host.py); and a two-object scene has a
tile-row whose retired run lies strictly between live tiles, which the one-interval fill of the
root cull could not write."""
import numpy as np
import pytest

import configs
import cull_fill_model as M
import retire_model as R
import tile_compact_model as C

SIZES = [(136, 72), (1024, 1024), (1160, 904)]       # 1160: 145 tile columns -- a partial mask word, an odd count, a narrow last column
_cache = {}


def _bunny(pkg):
    if "bunny" not in _cache:
        mesh, bvh, _ = pkg.prepare(configs.CONFIGS["bunny_1080"], arith=pkg.ARITH_FMA)
        _cache["bunny"] = (mesh, bvh, R.host_cut(pkg, mesh, bvh), M.root_box(mesh.tri))
    return _cache["bunny"]


def _two(pkg):
    if "two" not in _cache:
        mesh, bvh = R.two_patches(pkg)
        _cache["two"] = (mesh, bvh, R.host_cut(pkg, mesh, bvh), M.root_box(mesh.tri))
    return _cache["two"]


@pytest.mark.parametrize("W,H", SIZES)
def test_fill_runs_and_live_tiles_partition_every_frame(pkg, W, H):
    _, _, cut, root = _bunny(pkg)
    assert cut.n == 64 and cut.entry_ok == 1
    cams = C.cameras(pkg, root, W, H)
    names = ("odd", "gone", "inside", "centre")
    ret, rects = R.retired_tiles(pkg, cut, [cams[v] for v in names], root, W, H)
    culled = C.culled_tiles(rects, W, H)
    for f, v in enumerate(names):
        # buffer addresses that put heads and tails on the runs: frame f of a batch at 16 B + its offset
        R.check_partition(ret[f], W, H, px_addr=16 + 12 * f * W * H, rgb_addr=16 + 3 * f * W * H)
    assert ret[1].all(), "gone: every tile is root-culled"
    assert not ret[2].any(), "inside: every rectangle is keep, nothing is retired"
    for f in (0, 3):
        assert (ret[f] & ~culled[f]).any(), f"{names[f]}: no tile with an empty set S inside the root rectangle"
        assert (~ret[f]).any()


def _views():
    out = [(n, None) for n in ("dragon_333x217", "dragon_orbit3_333x217", "bunny_orbit7_160x120", "bunny_97x61_primary")]
    return out + [("dragon_333x217", f) for f in range(16)]


def test_no_hit_pixel_of_the_oracle_lies_in_a_retired_tile(pkg):
    import oracle
    views = _views()
    assert len(views) == 20
    scenes, checked = {}, 0
    for name, orbit in views:
        cfg = dict(configs.CONFIGS[name], mode="full")
        if orbit is not None:
            cfg.update(W=160, H=120)
        key = (name, orbit is not None)
        if key not in scenes:
            mesh, bvh, _ = pkg.prepare(configs.CONFIGS[name], arith=pkg.ARITH_FMA)
            scenes[key] = (oracle.prepare(cfg, contract=True), R.host_cut(pkg, mesh, bvh), M.root_box(mesh.tri))
        sc, cut, root = scenes[key]
        if orbit:
            eye, dir, sun = oracle.orbit(configs.BENCH_AXIS, 22.5, orbit, cfg["eye"], cfg["dir"], cfg["sun"], True)
            basis = oracle.camera_basis(eye, dir, cfg["up"], cfg["fov"], cfg["W"], cfg["H"], True)
        else:
            eye, sun, basis = sc["eye"], sc["sun"], sc["basis"]
        W, H = cfg["W"], cfg["H"]
        ref = oracle.render(sc, cfg, basis=basis, eye=eye, sun=sun, want_records=True, want_ppm=False, want_pixels=False)
        b12 = np.concatenate([np.asarray(eye, np.float32), np.asarray(basis, np.float32)])
        ret, _ = R.retired_tiles(pkg, cut, [b12], root, W, H)
        jj, ii = np.nonzero(ref["prim"].reshape(H, W) >= 0)
        assert len(jj), "the view hits nothing"
        assert not ret[0][jj // 8, ii // 8].any(), f"{name} orbit {orbit}: a hit pixel in a retired tile"
        R.check_partition(ret[0], W, H)
        checked += int(ret[0].sum())
    assert checked > 0


@pytest.mark.parametrize("W,H", [(136, 72), (1024, 1024)])
def test_two_objects_leave_a_retired_run_between_live_tiles(pkg, W, H):
    _, _, cut, root = _two(pkg)
    assert cut.n >= 2 and cut.entry_ok == 1
    b = C.look(pkg, root, W, H, dist=R.TWO_DIST)
    ret, rects = R.retired_tiles(pkg, cut, [b], root, W, H)
    rows = R.between_rows(ret[0])
    assert rows, "no tile-row with a retired run strictly between live tiles"
    culled = C.culled_tiles(rects, W, H)
    by = rows[0]
    assert not culled[0, by].all() and (ret[0, by] & ~culled[0, by]).any(), "the run between the objects is inside the root rectangle"
    n_runs = R.check_partition(ret[0], W, H, px_addr=16, rgb_addr=16)
    assert n_runs > 0


def test_group_flags_follow_the_compacted_order(pkg):
    """Flags over a source order compacted by tile_compact_model: only kept groups get a slot, a
    flagged slot's tiles are all retired, every other slot has a live tile."""
    _, _, cut, root = _two(pkg)
    W, H, tpw = 136, 72, 4
    b12 = [C.look(pkg, root, W, H, dist=R.TWO_DIST), C.look(pkg, root, W, H, dist=R.TWO_DIST, yaw=4.0)]
    ret, rects = R.retired_tiles(pkg, cut, b12, root, W, H)
    info = pkg.kept_tiles(W, H, len(b12), tpw, [list(r) for r in rects])
    src, packed, deal = info["source"], info["packed"], info["deal"]
    flags, keep = R.group_flags(src, packed, tpw, rects, ret, W, H, deal)
    order, tiles = C.compact(src, keep, tpw, deal)
    assert tiles == info["tiles"] and len(flags) == int(keep.sum())
    f, by, bx = C.decode(order[:tiles], packed, W, H)
    dead = ret[f, by, bx]
    for k in range(len(flags)):
        g = dead[k * tpw:(k + 1) * tpw]
        assert bool(flags[k]) == bool(g.all()), k
    assert flags.any() and not flags.all(), "a flagged group and a working group"
