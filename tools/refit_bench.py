#!/usr/bin/env python3
"""refit_bench.py -- what a refit costs beside recreating the scene, and what it does to the frame time.

For each config (default: the dragon of C3 and the C5 heightfield) the mesh is uploaded once, a device
scene is made the device way (ceres_bvh_build_device + ceres_scene_create_device) and the triangles are
deformed ON THE DEVICE (torch: the vertices p0, p0 - e1, p0 + e2 twisted about y by an angle proportional
to y and bent with a sine of x, in units of the mesh's largest half extent; {p0, e1, e2, cross(e1, e2)}
rebuilt).  Then, all on the host clock with the device idle before and after (both paths end synchronised):

  refit      Scene.refit_device(moved triangles, normals): the first call (which also sorts the records by
             level and allocates what later calls reuse) apart, then the median of --reps calls;
  recreate   the only alternative without it: build_bvh_device + Scene.from_device on the moved triangles
             + closing the old scene, median of --recreate-reps rounds.

The frame-time columns are the config's own view (single-frame render_device, median of --launches
launches between HIP events): the scene as built, after a refit to a MILD deformation, after a refit to a
VIOLENT one, and a scene REBUILT for the violent one -- the gap between the last two is the tree quality a
refit does not repair.

The upkeep columns (the same session, the same clocks): `sah_cost` is ceres_scene_sah_cost of the scene as
built, after the mild and the violent refit and after rebuilding for the violent mesh; `sah_cost_ms` one
such call (median of --reps, two launches and one synchronise); `rebuild_ms` the in-place
Scene.rebuild_device -- which ends with a cost measurement, the new baseline -- beside `recreate_ms`, the
path it replaces (median of --recreate-reps rounds each, min and max given); `update_keep` / `update_rebuild`
one Scene.update_device each on a fresh scene: the mild mesh with max_ratio = +inf (a refit and a
measurement, the scene's first refit included) and the violent mesh with a ratio that forces the rebuild.
`level_launches` is the number of per-level inner-box launches of one refit
(tree depth - 1).  Not part of bench.py; the numbers in DESIGN.md "Refit" come from this tool.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

MILD = dict(twist=0.15, bend=0.03)
VIOLENT = dict(twist=2.5, bend=0.4)


def deform_device(torch, d_tri, twist, bend):
    """The deformed [n, 12] float32 triangle records of d_tri, computed on the device."""
    p0 = d_tri[:, 0:3]
    V = torch.stack([p0, p0 - d_tri[:, 3:6], p0 + d_tri[:, 6:9]], dim=1)        # [n, 3, 3]
    lo, hi = V.amin(dim=(0, 1)), V.amax(dim=(0, 1))
    c, ext = (lo + hi) / 2, torch.clamp((hi - lo).max() / 2, min=1e-30)
    q = (V - c) / ext
    ang = twist * q[..., 1]
    x = torch.cos(ang) * q[..., 0] + torch.sin(ang) * q[..., 2]
    z = -torch.sin(ang) * q[..., 0] + torch.cos(ang) * q[..., 2]
    y = q[..., 1] + bend * torch.sin(3.0 * x)
    W = c + ext * torch.stack([x, y, z], dim=-1)
    P0, P1, P2 = W[:, 0], W[:, 1], W[:, 2]
    e1, e2 = P0 - P1, P2 - P0
    return torch.cat([P0, e1, e2, torch.linalg.cross(e1, e2)], dim=1).contiguous()


def median(v):
    return float(sorted(v)[len(v) // 2])


def bench_config(a, pkg, torch, name):
    cfg = pkg.configs.CONFIGS[name]
    W, H = cfg["W"], cfg["H"]
    mesh = pkg.proc_mesh(cfg["proc"]) if cfg.get("proc") else pkg.load_obj(pkg.configs.obj_path(cfg))
    if cfg.get("rotate"):
        pkg.rotate_triangles(mesh, cfg["rotate"][0], cfg["rotate"][1])
    n = len(mesh)
    cam, sun = pkg.pose(cfg)
    basis = cam.basis(W, H)
    mode = pkg.cfg_mode(cfg)
    d_tri = torch.from_numpy(mesh.tri).cuda()
    d_norm = torch.from_numpy(mesh.norm).cuda()
    del mesh
    d_nodes = torch.empty((2 * n - 1) * 8, dtype=torch.int32, device="cuda")
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda")
    d_rgb = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def create(tri):
        m = pkg.build_bvh_device(tri.data_ptr(), n, d_nodes.data_ptr(), d_prim.data_ptr(), sp)
        return pkg.Scene.from_device(tri.data_ptr(), n, d_norm.data_ptr(), d_nodes.data_ptr(), m, d_prim.data_ptr(), stream=sp)

    def frame_ms(scene):
        launch = lambda: scene.render_device(basis, sun, W, H, mode=mode, d_rgb8=d_rgb.data_ptr(), stream=sp)   # noqa: E731
        for _ in range(a.warmup):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for e0, e1 in ev:
            e0.record(stream)
            launch()
            e1.record(stream)
        stream.synchronize()
        return round(median([e0.elapsed_time(e1) for e0, e1 in ev]), 4)

    mild = deform_device(torch, d_tri, **MILD)
    violent = deform_device(torch, d_tri, **VIOLENT)
    torch.cuda.synchronize()
    scene = create(d_tri)
    info = scene.info()
    out = {"config": name, "W": W, "H": H, "n_tri": n, "n_pairs": info["n_pairs"], "depth": info["depth"],
           "level_launches": max(0, info["depth"] - 1), "frame_ms": {"built": frame_ms(scene)},
           "sah_cost": {"built": scene.sah_cost(sp)}}

    def refit(tri):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene.refit_device(tri.data_ptr(), d_norm.data_ptr(), stream=sp)       # synchronises `stream` itself
        return (time.perf_counter() - t0) * 1e3

    out["first_refit_ms"] = round(refit(mild), 4)
    out["frame_ms"]["refit_mild"] = frame_ms(scene)
    out["sah_cost"]["refit_mild"] = scene.sah_cost(sp)
    t = [refit(violent if k % 2 == 0 else mild) for k in range(a.reps + (a.reps + 1) % 2)]   # ends on the violent mesh
    out["refit_ms"] = {"median": round(median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4), "reps": len(t)}
    out["frame_ms"]["refit_violent"] = frame_ms(scene)
    out["sah_cost"]["refit_violent"] = scene.sah_cost(sp)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def spread(t):
        return {"median": round(median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4), "reps": len(t)}

    out["sah_cost_ms"] = spread([timed(lambda: scene.sah_cost(sp))[0] for _ in range(a.reps)])
    out["sah_cost_bytes_per_s"] = round(info["n_pairs"] * 64 / (out["sah_cost_ms"]["median"] * 1e-3), 0)
    # the alternative: a new BVH and a new scene for the moved triangles, the old scene closed
    t = []
    for k in range(a.recreate_reps):
        tri = violent if k % 2 == 0 else mild
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new = create(tri)
        scene.close()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
        scene = new
    out["recreate_ms"] = {"median": round(median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4), "reps": len(t)}
    # the same in place: the scene object, its stream, tile orders and workspaces stay
    t = [timed(lambda: scene.rebuild_device((violent if k % 2 == 0 else mild).data_ptr(), d_norm.data_ptr(), stream=sp))[0]
         for k in range(a.recreate_reps + (a.recreate_reps + 1) % 2)]                       # ends on the violent mesh
    out["rebuild_ms"] = spread(t)
    out["sah_cost"]["rebuilt_violent"] = scene.sah_cost(sp)
    out["frame_ms"]["rebuilt_in_place_violent"] = frame_ms(scene)
    scene.close()
    scene = create(d_tri)
    ms, u = timed(lambda: scene.update_device(mild.data_ptr(), float("inf"), d_norm.data_ptr(), stream=sp))
    out["update_keep"] = dict(u, ms=round(ms, 4))
    ms, u = timed(lambda: scene.update_device(violent.data_ptr(), 1e-9, d_norm.data_ptr(), stream=sp))
    out["update_rebuild"] = dict(u, ms=round(ms, 4))
    scene.close()
    scene = create(violent)
    out["frame_ms"]["rebuilt_violent"] = frame_ms(scene)
    scene.close()
    out["refit_speedup"] = round(out["recreate_ms"]["median"] / out["refit_ms"]["median"], 2)
    out["refit_bytes_per_s"] = round((n * (2 * 48 + 4 + 2 * 36) + info["n_pairs"] * 130) / (out["refit_ms"]["median"] * 1e-3), 0)
    print(f"{name}: {n} triangles, {info['n_pairs']} pairs, depth {info['depth']}: refit {out['refit_ms']['median']:.3f} ms "
          f"(first {out['first_refit_ms']:.3f}), recreate {out['recreate_ms']['median']:.3f} ms, rebuild in place "
          f"{out['rebuild_ms']['median']:.3f} ms, sah_cost {out['sah_cost_ms']['median']:.4f} ms; frame ms {out['frame_ms']}; "
          f"SAH cost {out['sah_cost']}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["dragon_1080", "proc_c5"])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--recreate-reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    from conftest import import_package
    pkg = import_package()
    if not torch.cuda.is_available():
        sys.exit("refit_bench.py needs the GPU (the CPU path: CpuScene.refit)")
    torch.cuda.set_device(a.device)
    result = {"version": pkg.lib().ceres_version().decode(), "reps": a.reps, "launches": a.launches,
              "deformations": {"mild": MILD, "violent": VIOLENT}, "configs": [bench_config(a, pkg, torch, c) for c in a.configs]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
