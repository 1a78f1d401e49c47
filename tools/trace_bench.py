#!/usr/bin/env python3
"""trace_bench.py -- throughput of the ray queries (ceres_trace_rays_device, --shade: ceres_shade_rays_device) on the C3 view.

Times the closest query and the any-hit query on the dragon 1920x1080 view's primary rays and on
the shadow rays of its hits, in three ray orders:
  tile     8x8 pixel tiles, tile after tile (a wavefront's 64 rays are one tile, as in the render kernels)
  row      row-major pixel order (a wavefront's rays are 64 neighbours of one row)
  shuffle  a fixed random permutation (incoherent wavefronts: what unsorted rays cost)
Shadow rays keep the order of the pixels they come from.  Every figure is the mean of --launches
(default 30, at least 20) launches between two HIP events on one stream after --warmup launches, no
counters passed.  Beside them: the primary-only render kernel (ceres_render_device, MODE_PRIMARY) on
the same view, which generates the same primary rays itself.  Not part of bench.py; the numbers in
DESIGN.md "Ray queries" come from this tool.  Contraction-free arithmetic (camera_rays / shadow_rays
build exactly the rays the exact render kernels trace).

--double runs the same orders on the config's double scene (ceres_trace_rays_f64_device: ray64 in,
hit32 out; camera_rays64 / shadow_rays64); the render figure beside them is the kernel time
(stats ms) of ceres_render_f64 in primary-only mode, mean of --launches host calls.

--all K[,K...] times the all-hits query (ceres_trace_rays_all_device) on the view's primary rays, in row
order and shuffled, for each K (0: the count-only kernel), beside the closest query on the same rays in
the same session: the median of --runs runs (default 9, at least 7; min and max listed) after --warmup,
each run --launches launches between two HIP events.  From a stats scene: node_pairs and tri_tests per
ray of both queries (the work the fixed window adds).  --cpu-threads T (default 16; 0: skip) times the
CPU path on the row-order rays.  --closest-only: the closest query alone, same rays and protocol (with
CERES_LIB=<another build's library>: that build's closest query, for a same-session comparison).

--lists times the complete-hit-list flow (the count-only ceres_trace_rays_all_device, ceres_hit_offsets_device,
ceres_trace_rays_lists_device: the fill kernel and the segment sort) on the view's primary rays, in row order
and shuffled, with --all's protocol: each step alone and the whole flow (without the read of the total, which
is taken once before the timing), ms per launch and Mrays/s, the records and the bytes written; like --all's
launches the timed ones pass no d_counters, and the fill call is timed once more with them.  --set NAME
--repeat R: instead of a view, the rays of tests/golden/rays_all/<NAME> repeated R times on that set's scene
(soup_mixed_nan_4097: lists of up to 987 records, where the sort shows).  --cpu-threads T times the CPU path.

--shade times the shaded ray query instead (ceres_shade_rays_device: closest hit, shadow ray and shading
in one launch) on the view's primary rays in row and in tile order, pixels out: the median of --launches
calls, each between its own pair of HIP events, after --warmup calls.  Beside it, on the same build:
  (a) the composition a caller needs without it, end to end on the host clock: trace_device(closest),
      hits to the host, shadow_rays in numpy, upload, trace_device(occluded), synchronise -- the host
      still has to shade; the two kernels' device times are listed apart;
  (b) one single-frame Scene.render_device of the same view (the tile kernel with work stealing, which
      generates its rays itself), the same way as the shaded query.
The shaded query's pixels are compared with render_device's, byte for byte, before anything is timed.

--ordered [--double]: the coherent ray order (ray_order_device) and the indexed queries beside the plain calls:
see ordered_bench.

--nearest: the closest-point query (ceres_closest_points_device) on the dragon and C5 meshes: see nearest_bench.
--nearest --double: the same protocol on the configs' double scenes (ceres_closest_points_f64_device: point32 in,
near32 out).

--double --shade: the same on the config's double scene (ceres_shade_rays_f64_device: ray64 in, 3 doubles
per ray out; camera_rays64 / shadow_rays64 for the composition).  A double scene has no device-pointer
render call, so (b) is the kernel time (stats ms) of ceres_render_f64 in full mode, median of --launches
host calls, and the pixels are compared with that call's framebuffer."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def orders(W, H, seed=12345):
    """Pixel permutations {name: index array over j*W + i}."""
    j, i = np.divmod(np.arange(W * H, dtype=np.int64), W)
    tiles_x = (W + 7) // 8
    key = ((j // 8) * tiles_x + i // 8) * 64 + (j % 8) * 8 + i % 8
    return {"tile": np.argsort(key, kind="stable"), "row": np.arange(W * H, dtype=np.int64),
            "shuffle": np.random.default_rng(seed).permutation(W * H)}


def shade_bench(a, pkg, torch):
    """--shade: see the module docstring.  Prints one JSON line."""
    import time
    cfg = pkg.configs.CONFIGS[a.config]
    W, H = cfg["W"], cfg["H"]
    n = W * H
    f64 = a.double
    mesh, bvh, cam = pkg.prepare(cfg, f64=f64)
    _, sun = pkg.pose_f64(cfg) if f64 else pkg.pose(cfg)
    basis = cam.basis(W, H)
    mode = pkg.MODE_ROBUST if cfg.get("robust") and not f64 else 0
    camera_rays, shadow_rays = (pkg.camera_rays64, pkg.shadow_rays64) if f64 else (pkg.camera_rays, pkg.shadow_rays)
    px_dt, hit_dt, hit_rec = (torch.float64, torch.int64, pkg.HIT64_DTYPE) if f64 else (torch.float32, torch.int32, pkg.HIT_DTYPE)
    scene = pkg.Scene(mesh, bvh, device=a.device)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def median_ms(launch, reps):
        for _ in range(a.warmup):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(stream)
            launch()
            e1.record(stream)
        stream.synchronize()
        t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return t[len(t) // 2], t[0], t[-1]

    prim = camera_rays(basis, W, H)
    d_px = torch.zeros(3 * n, dtype=px_dt, device="cuda")
    d_ref = torch.zeros(3 * n, dtype=px_dt, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_rays = torch.from_numpy(prim).cuda()
    torch.cuda.synchronize()
    if f64:
        d_ref = torch.from_numpy(scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)[0]).cuda()
    else:
        scene.render_device(basis, sun, W, H, mode=mode, d_pixels=d_ref.data_ptr(), stream=sp)
    scene.shade_device(d_rays.data_ptr(), n, sun, mode=mode, d_pixels=d_px.data_ptr(), d_counters=d_cnt.data_ptr(), stream=sp)
    stream.synchronize()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_px.view(hit_dt), d_ref.view(hit_dt)))
    cnt = d_cnt.cpu().numpy()
    result = {"config": a.config, "double": f64, "W": W, "H": H, "launches": a.launches, "warmup": a.warmup, "rays": int(cnt[0]),
              "hits": int(cnt[1]), "primary_rays": n, "shadow_rays": int(cnt[3]), "pixels_equal_render": same,
              "version": pkg.lib().ceres_version().decode(), "shade": {}}
    if not same:
        sys.exit("trace_bench.py --shade: the shaded query's pixels differ from the render call's")
    for name in ("row", "tile"):
        d_r = torch.from_numpy(np.ascontiguousarray(prim[orders(W, H)[name]])).cuda()
        torch.cuda.synchronize()
        med, lo, hi = median_ms(lambda: scene.shade_device(d_r.data_ptr(), n, sun, mode=mode, d_pixels=d_px.data_ptr(), stream=sp),
                                a.launches)
        result["shade"][name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                                 "mrays_s": round(int(cnt[0]) / med / 1e3, 1)}
        print(f"{a.config} {W}x{H} shade_device, {name} order: {med:.4f} ms (min {lo:.4f}, max {hi:.4f}) = "
              f"{int(cnt[0]) / med / 1e3:.1f} Mrays/s over {int(cnt[0])} rays (primary + shadow)")
    if f64:                                                           # no device-pointer render call in double
        for _ in range(a.warmup):
            scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)
        t = sorted(scene.render(basis, sun, W, H, mode=mode, want_rgb8=False)[2]["ms"] for _ in range(a.launches))
        med, lo, hi = t[len(t) // 2], t[0], t[-1]
    else:
        med, lo, hi = median_ms(lambda: scene.render_device(basis, sun, W, H, mode=mode, d_pixels=d_ref.data_ptr(), stream=sp),
                                a.launches)
    key, what = ("render_f64_kernel", "ceres_render_f64 full-mode kernel") if f64 else ("render_device", "single-frame render_device")
    result[key] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "mrays_s": round(int(cnt[0]) / med / 1e3, 1)}
    print(f"  (b) {what}: {med:.4f} ms (min {lo:.4f}, max {hi:.4f}) = {int(cnt[0]) / med / 1e3:.1f} Mrays/s")
    # (a) the composition, end to end
    d_hits = torch.empty((n, 4), dtype=hit_dt, device="cuda")
    wall, t_close, t_occ, t_host = [], [], [], []
    for k in range(a.warmup + max(5, a.launches // 6)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record(stream)
        scene.trace_device(d_rays.data_ptr(), n, mode=mode, d_hits16=d_hits.data_ptr(), stream=sp)
        e1.record(stream)
        stream.synchronize()
        hits = d_hits.cpu().numpy().view(hit_rec).reshape(-1)
        h0 = time.perf_counter()
        srays, idx = shadow_rays(mesh, hits, sun)
        h1 = time.perf_counter()
        d_s = torch.from_numpy(srays).cuda()
        d_occ = torch.empty(len(srays), dtype=torch.uint8, device="cuda")
        e2.record(stream)
        scene.trace_device(d_s.data_ptr(), len(srays), mode=mode, d_occluded=d_occ.data_ptr(), stream=sp)
        e3.record(stream)
        stream.synchronize()
        occ = d_occ.cpu().numpy()
        t1 = time.perf_counter()
        if k >= a.warmup:
            wall.append((t1 - t0) * 1e3); t_close.append(e0.elapsed_time(e1)); t_occ.append(e2.elapsed_time(e3))
            t_host.append((h1 - h0) * 1e3)
    assert len(idx) == int(cnt[3]) and int(occ.sum()) == int(cnt[1]) - int(cnt[3])
    med = lambda v: float(sorted(v)[len(v) // 2])                     # noqa: E731
    result["composition"] = {"calls": len(wall), "end_to_end_ms": round(med(wall), 3), "closest_kernel_ms": round(med(t_close), 4),
                             "occluded_kernel_ms": round(med(t_occ), 4), "host_shadow_rays_ms": round(med(t_host), 3)}
    print(f"  (a) trace(closest) + host shadow_rays + trace(occluded), end to end: {med(wall):.3f} ms "
          f"(kernels {med(t_close):.4f} + {med(t_occ):.4f} ms, numpy shadow_rays {med(t_host):.3f} ms; shading still to do)")
    scene.close()
    print(json.dumps(result))


def all_hits_bench(a, pkg, torch):
    """--all / --closest-only: see the module docstring.  Prints one JSON line."""
    cfg = pkg.configs.CONFIGS[a.config]
    W, H = cfg["W"], cfg["H"]
    n = W * H
    ks = [] if a.closest_only else [int(k) for k in a.all.split(",")]
    if any(k < 0 or k > 32 for k in ks):
        sys.exit("trace_bench.py --all: K in 0 .. 32 (0: count-only)")
    mesh, bvh, cam = pkg.prepare(cfg, f64=a.double)
    prim = (pkg.camera_rays64 if a.double else pkg.camera_rays)(cam.basis(W, H), W, H)
    scene = pkg.Scene(mesh, bvh, device=a.device)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    runs = max(7, a.runs)

    def timed(launch):
        for _ in range(a.warmup):
            launch()
        t = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.launches):
                launch()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / a.launches)
        t.sort()
        return {"ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                "mrays_s": round(n / t[len(t) // 2] / 1e3, 1)}

    result = {"config": a.config, "double": a.double, "W": W, "H": H, "rays": n, "launches": a.launches, "runs": runs, "warmup": a.warmup,
              "version": pkg.lib().ceres_version().decode(), "lib": os.path.relpath(pkg.LIB_PATH, REPO), "orders": {}}
    rec_dt = torch.int64 if a.double else torch.int32                 # a hit32 record: 4 x 8 B, a hit16 record: 4 x 4 B
    d_hits = torch.empty((n, 4), dtype=rec_dt, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    d_rows = torch.empty((n * max(ks + [1]), 4), dtype=rec_dt, device="cuda")
    perms = orders(W, H)
    for name in ("row", "shuffle"):
        d_rays = torch.from_numpy(np.ascontiguousarray(prim[perms[name]])).cuda()
        torch.cuda.synchronize()
        row = {"closest": timed(lambda: scene.trace_device(d_rays.data_ptr(), n, d_hits16=d_hits.data_ptr(), stream=sp))}
        print(f"{a.config} {W}x{H} {name:8s} closest    : {row['closest']}")
        for k in ks:
            if k:
                launch = lambda: scene.trace_all_device(d_rays.data_ptr(), n, max_hits=k, d_counts=d_cnt.data_ptr(),   # noqa: E731
                                                        d_hits16=d_rows.data_ptr(), stream=sp)
            else:
                launch = lambda: scene.trace_all_device(d_rays.data_ptr(), n, d_counts=d_cnt.data_ptr(), stream=sp)    # noqa: E731
            key = "all_%d" % k if k else "all_count_only"
            row[key] = timed(launch)
            row[key]["vs_closest"] = round(row[key]["ms"] / row["closest"]["ms"], 3)
            print(f"{a.config} {W}x{H} {name:8s} {key:11s}: {row[key]}")
        result["orders"][name] = row
    scene.close()
    if ks:
        st_scene = pkg.Scene(mesh, bvh, device=a.device, stats=True)
        _, _, sc = st_scene.trace(prim)
        counts, _, sa = st_scene.trace_all(prim, hits=False)
        st_scene.close()
        result["work_per_ray"] = {"closest_node_pairs": round(sc["node_pairs"] / n, 3), "all_node_pairs": round(sa["node_pairs"] / n, 3),
                                  "closest_tri_tests": round(sc["tri_tests"] / n, 3), "all_tri_tests": round(sa["tri_tests"] / n, 3),
                                  "step_ratio": round(sa["node_pairs"] / sc["node_pairs"], 3), "rays_with_a_hit": int(sa["hits"]),
                                  "mean_count_of_hit_rays": round(float(counts[counts > 0].mean()), 3), "max_count": int(counts.max()),
                                  "rays_with_count_over_8": int((counts > 8).sum()), "rays_with_count_over_32": int((counts > 32).sum())}
        print("work per ray:", result["work_per_ray"])
        if a.cpu_threads > 0:
            cpu = pkg.CpuScene(mesh, bvh)
            cpu.trace(prim, threads=a.cpu_threads)
            row = {"threads": a.cpu_threads}
            ms = sorted(cpu.trace(prim, threads=a.cpu_threads)[2]["ms"] for _ in range(3))
            row["closest"] = {"ms": round(ms[1], 2), "mrays_s": round(n / ms[1] / 1e3, 2)}
            for k in ks:
                ms = sorted(cpu.trace_all(prim, max_hits=max(k, 1), hits=k > 0, threads=a.cpu_threads)[2]["ms"] for _ in range(3))
                row["all_%d" % k if k else "all_count_only"] = {"ms": round(ms[1], 2), "mrays_s": round(n / ms[1] / 1e3, 2)}
            cpu.close()
            result["cpu"] = row
            print("CPU path:", row)
    print(json.dumps(result))


def lists_bench(a, pkg, torch):
    """--lists: see the module docstring.  Prints one JSON line."""
    if a.set and a.double:
        sys.exit("trace_bench.py --lists --set: the stored sets are float scenes (--double takes the config's view)")
    rec_dt, rec_bytes = (torch.int64, 32) if a.double else (torch.int32, 16)
    if a.set:
        import allhits_common as ac
        mesh, bvh = ac.all_set_scene(a.set, 0)
        base = np.tile(ac.load_all_fixture(a.set)["rays"], (max(1, a.repeat), 1))
        label, mode = "%s x %d" % (a.set, max(1, a.repeat)), 0
    else:
        cfg = pkg.configs.CONFIGS[a.config]
        W, H = cfg["W"], cfg["H"]
        mesh, bvh, cam = pkg.prepare(cfg, f64=a.double)
        base = (pkg.camera_rays64 if a.double else pkg.camera_rays)(cam.basis(W, H), W, H)
        label, mode = "%s %dx%d%s" % (a.config, W, H, " double" if a.double else ""), 0   # --all's scene and mode
    n = len(base)
    scene = pkg.Scene(mesh, bvh, device=a.device)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    runs = max(7, a.runs)

    def timed(launch):
        for _ in range(a.warmup):
            launch()
        t = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.launches):
                launch()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / a.launches)
        t.sort()
        return {"ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                "mrays_s": round(n / t[len(t) // 2] / 1e3, 1)}

    result = {"rays_of": label, "rays": n, "mode": mode, "launches": a.launches, "runs": runs, "warmup": a.warmup,
              "version": pkg.lib().ceres_version().decode(), "lib": os.path.relpath(pkg.LIB_PATH, REPO),
              "list_entries": os.environ.get("CERES_DEBUG_LIST_ENTRIES", "default"),
              "sort_cap": os.environ.get("CERES_DEBUG_LIST_SORT_CAP", "default"), "orders": {}}
    nbytes = pkg.hit_offsets_scratch_bytes(n)
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_scr = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
    perms = {"row": np.arange(n), "shuffle": np.random.default_rng(12345).permutation(n)}
    for name in ("row", "shuffle"):
        d_rays = torch.from_numpy(np.ascontiguousarray(base[perms[name]])).cuda()
        torch.cuda.synchronize()
        count = lambda: scene.trace_all_device(d_rays.data_ptr(), n, mode=mode, d_counts=d_cnt.data_ptr(), stream=sp)   # noqa: E731
        scan = lambda: scene.hit_offsets_device(d_cnt.data_ptr(), n, d_off.data_ptr(), d_scr.data_ptr(), nbytes, stream=sp)   # noqa: E731
        count()
        scan()
        stream.synchronize()
        total = int(d_off[n].item())
        d_hits = torch.empty((max(total, 1), 4), dtype=rec_dt, device="cuda")
        fill = lambda: scene.trace_lists_device(d_rays.data_ptr(), n, d_off.data_ptr(), d_hits.data_ptr(), total, mode=mode, stream=sp)   # noqa: E731
        # ... and with d_counters, as a caller that wants the flags pays it: two atomics per wavefront that walks
        fill_ctr = lambda: scene.trace_lists_device(d_rays.data_ptr(), n, d_off.data_ptr(), d_hits.data_ptr(), total, mode=mode,   # noqa: E731
                                                    d_counters=d_ctr.data_ptr(), stream=sp)
        # (the call launches the fill kernel and the segment sort; a kernel trace of this tool lists them apart)
        def flow():
            count()
            scan()
            fill()
        row = {"count_only": timed(count), "scan": timed(scan), "fill_and_sort": timed(fill), "flow": timed(flow),
               "fill_and_sort_with_counters": timed(fill_ctr)}
        stream.synchronize()
        c = d_ctr.cpu().numpy()
        counts = d_cnt.cpu().numpy().view(np.uint32)
        row.update(records=total, record_bytes=total * rec_bytes, offset_bytes=(n + 1) * 8, rays_walked=int(c[1]), flags=[int(c[6]), int(c[7])],
                   rays_past_list=int((counts > 8).sum()), max_count=int(counts.max()))
        for k, v in row.items():
            print(f"{label} {name:8s} {k:14s}: {v}")
        result["orders"][name] = row
        del d_hits
    scene.close()
    if a.cpu_threads > 0:
        cpu = pkg.CpuScene(mesh, bvh)
        cpu.trace_lists(base, mode=mode, threads=a.cpu_threads)
        ms = sorted(cpu.trace_lists(base, mode=mode, threads=a.cpu_threads)[2]["ms"] for _ in range(3))
        result["cpu"] = {"threads": a.cpu_threads, "ms": round(ms[1], 2), "mrays_s": round(n / ms[1] / 1e3, 2),
                         "note": "Scene.trace_lists calls the C entry twice (size, then fill); ms is the second call's"}
        cpu.close()
        print("CPU path:", result["cpu"])
    print(json.dumps(result))


def ordered_bench(a, pkg, torch):
    """--ordered: the coherent order and the indexed queries on the config's primary rays, the closest query
    and the count-only all-hits query each, --all's protocol (warm-up, then --runs runs of --launches
    launches between two events: median, min, max):
      (a) the plain call on shuffled rays;          (b) ray_order_device alone (shuffled rays);
      (c) the indexed call with that order;         (d) (b) + (c) in one stream;
      (e) the plain call in row order and in 8 x 8 tiles (the ceiling);
      (f) the indexed call with the identity list on row-order rays (the price of the indirection).
    Prints one JSON line."""
    cfg = pkg.configs.CONFIGS[a.config]
    W, H = cfg["W"], cfg["H"]
    n = W * H
    mesh, bvh, cam = pkg.prepare(cfg, f64=a.double)
    prim = (pkg.camera_rays64 if a.double else pkg.camera_rays)(cam.basis(W, H), W, H)
    scene = pkg.Scene(mesh, bvh, device=a.device)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    runs = max(7, a.runs)

    def timed(launch):
        for _ in range(a.warmup):
            launch()
        t = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.launches):
                launch()
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / a.launches)
        t.sort()
        return {"ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                "mrays_s": round(n / t[len(t) // 2] / 1e3, 1)}

    rec_dt = torch.int64 if a.double else torch.int32
    d_hits = torch.empty((n, 4), dtype=rec_dt, device="cuda")
    d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    d_order = torch.empty(n, dtype=torch.int32, device="cuda")
    d_iota = torch.arange(n, dtype=torch.int32, device="cuda")
    nb = pkg.ray_order_scratch_bytes(n)
    d_scr = torch.empty(nb, dtype=torch.uint8, device="cuda")
    perms = orders(W, H)
    d_rays = {k: torch.from_numpy(np.ascontiguousarray(prim[perms[k]])).cuda() for k in ("row", "tile", "shuffle")}
    torch.cuda.synchronize()

    def order(rays):
        scene.ray_order_device(rays.data_ptr(), n, d_order.data_ptr(), d_scr.data_ptr(), nb, stream=sp)

    queries = {"closest": lambda rays, **ix: scene.trace_device(rays.data_ptr(), n, d_hits16=d_hits.data_ptr(), stream=sp, **ix),
               "all_count_only": lambda rays, **ix: scene.trace_all_device(rays.data_ptr(), n, d_counts=d_cnt.data_ptr(), stream=sp, **ix)}
    result = {"config": a.config, "double": a.double, "W": W, "H": H, "rays": n, "launches": a.launches, "runs": runs, "warmup": a.warmup,
              "version": pkg.lib().ceres_version().decode(), "scratch_bytes": nb, "cells": {}}
    sh = d_rays["shuffle"]
    result["cells"]["b_order_alone"] = timed(lambda: order(sh))
    print(f"{a.config} {W}x{H} (b) order alone: {result['cells']['b_order_alone']}")
    order(sh)
    stream.synchronize()
    for name, q in queries.items():
        ix = dict(d_index=d_order.data_ptr(), n_index=n)
        row = {"a_plain_shuffled": timed(lambda: q(sh)),
               "c_indexed_ordered": timed(lambda: q(sh, **ix)),
               "d_order_plus_indexed": timed(lambda: (order(sh), q(sh, **ix))),
               "e_plain_row": timed(lambda: q(d_rays["row"])),
               "e_plain_tile": timed(lambda: q(d_rays["tile"])),
               "f_indexed_identity_row": timed(lambda: q(d_rays["row"], d_index=d_iota.data_ptr(), n_index=n))}
        result["cells"][name] = row
        for k, v in row.items():
            print(f"{a.config} {W}x{H} {name:15s} {k:24s}: {v}")
    scene.close()
    print(json.dumps(result))


def morton_order(torch, d_points, lo, hi):
    """The permutation that sorts points [n, 4] (a device tensor) by the 30-bit Morton code of their cell on a
    1024^3 grid over [lo, hi] -- computed with torch (ceres_ray_order_device takes rays, not points)."""
    span = torch.clamp(hi - lo, min=1e-30)
    q = torch.clamp(((d_points[:, :3] - lo) / span * 1024).to(torch.int64), 0, 1023)

    def spread(x):                                                    # 10 bits -> every third bit
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249

    key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.argsort(key, stable=True).to(torch.int32)


def nearest_bench(a, pkg, torch):
    """--nearest: the closest-point query (ceres_closest_points_device) on dragon and C5, --all's protocol
    (warm-up, then --runs runs of --launches launches between two events: median, min, max).  The points are a
    --grid^3 lattice through 1.2 x the mesh's bounding box, r2max = +inf, in three forms:
      grid      lattice order (x fastest);
      shuffle   a fixed random permutation of them;
      morton    the shuffled array through the indexed call with its Morton order (the sort is not timed).
    Beside them: node pairs and triangle tests per point from a stats scene (grid and shuffle; a stats scene has
    no indexed call), and the CPU path on the shuffled points with --cpu-threads threads.  --double: the configs'
    double scenes, float64 points, the _f64 calls.  One JSON line."""
    runs = max(7, a.runs)
    f64 = a.double
    np_dt, t_dt, rec_dt = (np.float64, torch.float64, torch.int64) if f64 else (np.float32, torch.float32, torch.int32)
    result = {"double": f64, "lib": os.path.relpath(pkg.LIB_PATH, REPO), "grid": a.grid, "launches": a.launches, "runs": runs, "warmup": a.warmup,
              "version": pkg.lib().ceres_version().decode(), "scenes": {}}
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    for config in a.nearest_configs.split(","):
        cfg = pkg.configs.CONFIGS[config]
        mesh, bvh, _ = pkg.prepare(cfg, f64=f64)
        v = np.concatenate([mesh.tri[:, 0:3], mesh.tri[:, 0:3] - mesh.tri[:, 3:6], mesh.tri[:, 0:3] + mesh.tri[:, 6:9]])
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        c, h = (lo + hi) / 2, 0.6 * (hi - lo)
        ax = [np.linspace(c[k] - h[k], c[k] + h[k], a.grid) for k in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        pts = np.stack([x.ravel(), y.ravel(), z.ravel(), np.full(x.size, np.inf)], axis=1).astype(np_dt)
        n = len(pts)
        shuffled = pts[np.random.default_rng(12345).permutation(n)]
        d_pts = {"grid": torch.from_numpy(pts).cuda(), "shuffle": torch.from_numpy(shuffled).cuda()}
        d_out = torch.empty((n, 4), dtype=rec_dt, device="cuda")          # a near16 record: 4 x 4 B, a near32 record: 4 x 8 B
        d_cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
        t_lo, t_hi = (torch.tensor(c - h, dtype=t_dt, device="cuda"), torch.tensor(c + h, dtype=t_dt, device="cuda"))
        d_order = morton_order(torch, d_pts["shuffle"], t_lo, t_hi)
        scene = pkg.Scene(mesh, bvh, device=a.device)
        device_call = lambda sc: sc.closest_points_f64_device if f64 else sc.closest_points_device   # noqa: E731
        torch.cuda.synchronize()

        def timed(launch):
            for _ in range(a.warmup):
                launch()
            t = []
            for _ in range(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.launches):
                    launch()
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1) / a.launches)
            t.sort()
            return {"ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                    "mpoints_s": round(n / t[len(t) // 2] / 1e3, 1)}

        row = {"triangles": len(mesh), "points": n, "info": scene.info()}
        for k in ("grid", "shuffle"):
            row[k] = timed(lambda: device_call(scene)(d_pts[k].data_ptr(), n, d_out.data_ptr(), stream=sp))
        row["morton"] = timed(lambda: device_call(scene)(d_pts["shuffle"].data_ptr(), n, d_out.data_ptr(), stream=sp,
                                                         d_index=d_order.data_ptr(), n_index=n))
        want = d_out.cpu().numpy().copy()                             # (the indexed call's answers, in the shuffled slots)
        device_call(scene)(d_pts["shuffle"].data_ptr(), n, d_out.data_ptr(), stream=sp)
        stream.synchronize()
        assert np.array_equal(want, d_out.cpu().numpy()), "the indexed call's answers differ from the plain call's"
        scene.close()
        stats = pkg.Scene(mesh, bvh, device=a.device, stats=True)
        for k in ("grid", "shuffle"):
            device_call(stats)(d_pts[k].data_ptr(), n, d_out.data_ptr(), d_counters=d_cnt.data_ptr(), stream=sp)
            stream.synchronize()
            cn = d_cnt.cpu().numpy()
            row[k]["node_pairs_per_point"] = round(float(cn[4]) / n, 2)
            row[k]["tri_tests_per_point"] = round(float(cn[5]) / n, 2)
            row[k]["found"] = int(cn[1])
        stats.close()
        if a.cpu_threads > 0:
            cpu = pkg.CpuScene(mesh, bvh)
            cpu_call = cpu.closest_points_f64 if f64 else cpu.closest_points
            got, st = cpu_call(shuffled, threads=a.cpu_threads)
            t = sorted(cpu_call(shuffled, threads=a.cpu_threads)[1]["ms"] for _ in range(3))
            assert np.array_equal(got.view(np.int64 if f64 else np.int32).reshape(-1, 4), d_out.cpu().numpy()), \
                "the CPU path's answers differ from the GPU's"
            row["cpu"] = {"threads": a.cpu_threads, "ms": round(t[1], 2), "mpoints_s": round(n / t[1] / 1e3, 2),
                          "node_pairs_per_point": round(st["node_pairs"] / n, 2), "tri_tests_per_point": round(st["tri_tests"] / n, 2)}
            cpu.close()
        result["scenes"][config] = row
        for k, val in row.items():
            print(f"{config} {k:10s}: {val}", flush=True)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="dragon_1080")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--double", action="store_true", help="the config's double scene (ceres_trace_rays_f64_device)")
    ap.add_argument("--shade", action="store_true", help="the shaded ray query (ceres_shade_rays_device) beside its alternatives")
    ap.add_argument("--all", default="", metavar="K[,K...]", help="the all-hits query (ceres_trace_rays_all_device); 0: count-only")
    ap.add_argument("--lists", action="store_true", help="the complete-hit-list flow (count, scan, fill and sort)")
    ap.add_argument("--set", default="", help="--lists: a ray set of tests/golden/rays_all/ instead of the config's view")
    ap.add_argument("--repeat", type=int, default=1, help="--lists --set: the set's rays repeated this many times")
    ap.add_argument("--closest-only", action="store_true", help="--all's protocol for the closest query alone")
    ap.add_argument("--ordered", action="store_true", help="the coherent order and the indexed queries against the plain calls")
    ap.add_argument("--runs", type=int, default=9, help="--all: timed runs (median, min, max)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="--all: threads of the CPU-path timing (0: skip)")
    ap.add_argument("--nearest", action="store_true", help="the closest-point query (ceres_closest_points_device) on dragon and C5")
    ap.add_argument("--nearest-configs", default="dragon_1080,proc_c5", help="--nearest: the configs whose meshes are queried")
    ap.add_argument("--grid", type=int, default=100, help="--nearest: points per axis of the lattice")
    a = ap.parse_args()
    if a.all or a.closest_only or a.lists or a.ordered or a.nearest:
        a.launches = max(1, a.launches)
    else:
        a.launches = max(20, a.launches)
    import torch
    from conftest import import_package
    pkg = import_package()
    if not torch.cuda.is_available():
        sys.exit("trace_bench.py needs the GPU (the CPU path: CpuScene.trace)")
    torch.cuda.set_device(a.device)
    if a.ordered:
        return ordered_bench(a, pkg, torch)
    if a.nearest:
        return nearest_bench(a, pkg, torch)
    if a.shade:
        return shade_bench(a, pkg, torch)
    if a.lists:
        return lists_bench(a, pkg, torch)
    if a.all or a.closest_only:
        return all_hits_bench(a, pkg, torch)
    cfg = pkg.configs.CONFIGS[a.config]
    W, H = cfg["W"], cfg["H"]
    mesh, bvh, cam = pkg.prepare(cfg, f64=a.double)
    _, sun = pkg.pose_f64(cfg) if a.double else pkg.pose(cfg)
    basis = cam.basis(W, H)
    camera_rays, shadow_rays = (pkg.camera_rays64, pkg.shadow_rays64) if a.double else (pkg.camera_rays, pkg.shadow_rays)
    scene = pkg.Scene(mesh, bvh, device=a.device)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def timed(launch):
        for _ in range(a.warmup):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.launches):
            launch()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches

    prim = camera_rays(basis, W, H)
    hits, _, st = scene.trace(prim)
    assert st["rays"] == W * H
    result = {"config": a.config, "double": a.double, "W": W, "H": H, "launches": a.launches, "primary_rays": W * H,
              "primary_hits": int(st["hits"]), "version": pkg.lib().ceres_version().decode(), "orders": {}}
    if a.double:                                                      # no device-pointer render call in double
        for _ in range(a.warmup):
            scene.render(basis, sun, W, H, mode=pkg.MODE_PRIMARY, want_rgb8=False)
        ms = float(np.mean([scene.render(basis, sun, W, H, mode=pkg.MODE_PRIMARY, want_rgb8=False)[2]["ms"]
                            for _ in range(a.launches)]))
    else:
        d_px = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
        ms = timed(lambda: scene.render_device(basis, sun, W, H, mode=pkg.MODE_PRIMARY, d_pixels=d_px.data_ptr(), stream=sp))
    result["render_primary_only_ms"] = round(ms, 4)
    result["render_primary_only_mrays_s"] = round(W * H / ms / 1e3, 1)
    print(f"{a.config} {W}x{H}: primary-only render kernel {ms:.4f} ms = {W * H / ms / 1e3:.1f} Mrays/s "
          f"({st['hits']} of {W * H} primary rays hit)")
    for name, perm in orders(W, H).items():
        p = np.ascontiguousarray(prim[perm])
        srays, _ = shadow_rays(mesh, hits[perm], sun)
        row = {}
        for kind, rays in (("primary", p), ("shadow", srays)):
            n = len(rays)
            d_rays = torch.from_numpy(rays).cuda()
            d_hits = torch.empty((n, 4), dtype=torch.int64 if a.double else torch.int32, device="cuda")
            d_occ = torch.empty(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t_c = timed(lambda: scene.trace_device(d_rays.data_ptr(), n, d_hits16=d_hits.data_ptr(), stream=sp))
            t_a = timed(lambda: scene.trace_device(d_rays.data_ptr(), n, d_occluded=d_occ.data_ptr(), stream=sp))
            row[kind] = {"rays": n, "closest_ms": round(t_c, 4), "closest_mrays_s": round(n / t_c / 1e3, 1),
                         "any_ms": round(t_a, 4), "any_mrays_s": round(n / t_a / 1e3, 1),
                         "occluded": int(d_occ.sum().item())}
            print(f"  {name:8s} {kind:8s} {n:8d} rays: closest {t_c:8.4f} ms = {n / t_c / 1e3:9.1f} Mrays/s   "
                  f"any-hit {t_a:8.4f} ms = {n / t_a / 1e3:9.1f} Mrays/s")
        result["orders"][name] = row
    scene.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
