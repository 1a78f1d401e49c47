// render_cli.cpp -- the `./render <obj> --eye ... --rotate ...` CLI of README.md:11.
//
// The reference documents this CLI but never built it (include/CMakeLists.txt:1 comments the
// target out; static.cpp:21-24 ignores argv).  This is its MI355X implementation: the
// static.cpp sequence (load :76, rotate :83-88, BVH :100-107, render :130, PPM :135-147) with
// the hot path on the GPU through libceres_hip.so.  Defaults follow static.cpp:39-47,72-73.
//
//   render <obj> [--eye x y z] [--dir x y z] [--up x y z] [--fov deg] [--sun x y z]
//                [--rotate x|y|z deg] [--size W H] [-o|--out file.ppm] [--primary-only]
//                [--proc N] [--device D] [--bench reps] [--json]
//                [--orbit ax ay az step_deg count] [--frames N] [--gpu-bvh] [--double|-d]
//                [--gpus N] [--row-block R] [--robust] [--qbvh] [--exact | --fma] [--cpu [--threads T]]
//                [--refit B.obj [--rebuild-above R]]
//
// Arithmetic (float and double pipelines): --fma (the default) computes every step as the reference's own
// CMake build does (CMakeLists.txt:11-13, g++ -O3 -mavx2 -mfma: GCC contracts a*b+c into FMA at
// the sites listed in oracle/contraction_sites.txt) -- the scene (normals, rotation, SAH costs),
// the camera basis, the orbit and the kernels (CERES_ARITH_FMA + CERES_MODE_FMA), so the PPM is
// the one that build writes.  --exact is the contraction-free reference (-ffp-contract=off).
//
// --robust traverses with the library's RobustNodeIntersector (node_intersectors.hpp:54-79,
// T. Ize's padded-inverse slab test) instead of render()'s FastNodeIntersector.
//
// --gpus N splits every frame over N GPUs of this node in one process: rows
// are dealt in blocks of R (default 8) rows round-robin to ranks on devices D, D+1, ... (mod
// the device count, so N > devices reuses devices -- the test mode on a one-GPU box), each
// rank with its own scene copy; the RGB8 rows are gathered peer-to-peer over xGMI to the first
// device and assembled there (ceres_render_multi_f32).  The PPM is identical to --gpus 1.
//
// --double (anim.cpp's -d, anim.cpp:146-155) runs the whole sequence as render<double>:
// numbers parsed with strtod, double mesh / BVH / camera, the double GPU kernel.
// --gpu-bvh builds the same BinnedSahBuilder BVH with the gfx950 builder (bvh_build.hip; with --double:
// bvh_build64.hip).
//
// --orbit / --frames are the anim.cpp:76-125 driver without Magick++: the camera eye, dir and
// the sun are rotated by step_deg about the axis (transform.hpp:67-112) `count` times before
// the first frame, and once more per further frame; N frames are written as
// <out-stem>_000.ppm ... (one file when N = 1), "Total Rays" summed like anim.cpp:127.
//
// --cpu renders on the host cores instead (ceres_render_cpu_f32 / _f64: the product's CPU path, the
// same images, rays and hits, float or --double; one process; --threads T, default the OpenMP default) --
// SURVEY.md §7 step 3's "config 1 works with no GPU".  It is only ever chosen by the flag:
//
// --rays FILE traces the file's raw ray32 records ({origin, direction, tmin, tmax}, 32 B each:
// bvh::Ray<float>) against the scene instead of rendering a picture (ceres_trace_rays, or
// ceres_trace_rays_cpu with --cpu): --hits-out gets the closest hits as raw hit16 records ({int32
// original triangle or -1, t, u, v}), --occluded-out one 0 / 1 byte per ray; --json prints rays,
// hits and ms.  A file that is not a whole number of records is bad usage (status 2).  With --double
// the file holds ray64 records (bvh::Ray<double>, 64 B each) and --hits-out gets hit32 records ({int32
// original triangle or -1, uint32 0, double t, u, v}): ceres_trace_rays_f64 / ceres_trace_rays_cpu_f64.
//
// --coherent (the plain ray query on the GPU only) traces the rays in the coherent order the library
// computes (ceres_trace_rays_coherent / _f64): the output files are byte-identical.
//
// --rays FILE with --all-hits K is the all-hits query (ceres_trace_rays_all, or ceres_trace_rays_all_cpu
// with --cpu): every hit in each ray's window, the K smallest by (t, original triangle) as K hit16
// records per ray, ray after ray, in --hits-out (padded with misses), the size of each ray's hit set as
// a raw uint32 in --counts-out.  K = 0 with --counts-out alone is the count-only query.  Float scenes
// only: with --double the library's refusal, status 1.
//
// --rays FILE with --hit-lists-out FILE and --offsets-out FILE (both required) is the complete-hit-list
// query (ceres_trace_rays_lists, or ceres_trace_rays_lists_cpu with --cpu): every hit of every ray, without
// a cap -- each ray's whole set in the order above as hit16 records, ray after ray without padding, in
// --hit-lists-out, and the n + 1 raw uint64 offsets of the rays' segments in --offsets-out.  Not with
// --all-hits, --hits-out, --occluded-out or the shaded outputs (bad usage); float scenes only.
//
// --rays FILE with --pixels-out, --rgb8-out or --status-out is the shaded query (ceres_shade_rays, or
// ceres_shade_rays_cpu with --cpu): render()'s pixel for every ray of the file under --sun, written as
// raw arrays in ray order -- --pixels-out 3 floats per ray, --rgb8-out 3 bytes per ray (the PPM
// quantiser, no row flip), --status-out one byte per ray (0 miss, 1 lit, 2 in shadow), --hits-out the
// closest hits as above.  With --double (ceres_shade_rays_f64 / ceres_shade_rays_cpu_f64) the file holds
// ray64 records, --pixels-out gets 3 doubles per ray and --hits-out hit32 records.
//
// --refit B.obj builds the BVH on <obj>, then refits the scene in place to B's triangles and normals
// (ceres_scene_refit / ceres_cpu_scene_refit and their _f64 siblings: topology kept, every box
// recomputed) and renders or traces B.  B is loaded and rotated like <obj> and must have the same face
// count (otherwise an error, status 1).  With --cpu, --double, --rays, --gpus.
//
// --rebuild-above R (only with --refit, otherwise bad usage) makes that step the update call
// (ceres_scene_update / ceres_cpu_scene_update and its _f64 sibling) with max_ratio = R: refit, measure
// the SAH cost, and rebuild the tree in place when the cost exceeds R times the cost of <obj>'s tree; one
// line reports the cost, the baseline, their ratio and `rebuilt` or `kept` (per rank with --gpus).  A GPU
// --double scene cannot be rebuilt: the library's message, status 1.
//
// --points FILE with --nearest-out FILE is the closest-point query (ceres_closest_points, or
// ceres_closest_points_cpu with --cpu): the file's raw point16 records ({x, y, z, r2max}, 16 B each) in,
// one raw near16 record ({int32 prim, float d2, u, v}) per point out.  Float scenes only: with --double
// the library's refusal, status 1.  Not with --rays or any of its outputs (bad usage).
//
// Exit status: 0 on success, 1 on a load/render error (message on stderr), 2 on bad usage.
// There is no CPU fallback: without --cpu and without a gfx950 device the render step fails.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cctype>
#include <type_traits>

#include "ceres_render.h"

namespace {

// Every number is kept as float (strtof, render<float>) and as double (strtod: the double
// literals of anim.cpp's -d mode); --double selects the double pipeline.
template <class S> struct Num {
    S eye[3] = {0, -15, 2}, dir[3] = {0, 1, 0}, up[3] = {0, 0, 1}, sun[3] = {-50, -20, 0};
    S fov = 60, rot_deg = 0, orbit_axis[3] = {0, 1, 0}, orbit_step = 0;
};

struct Opts {
    std::string obj, out = "render.ppm";
    std::string refit;                             // --refit: refit the scene to this OBJ's triangles before rendering
    bool rebuild = false;                          // --rebuild-above R: the refit step is the update call ...
    double rebuild_above = 0;                      // ... with max_ratio = R
    Num<float> f;
    Num<double> d;
    int rot_axis = -1;
    size_t W = 1920, H = 1080;
    int mode = CERES_MODE_FULL, proc = 0, device = 0, bench = 0, gpus = 1, row_block = 16;
    bool json = false, gpu_bvh = false, f64 = false;
    int arith = CERES_ARITH_FMA;                   // --fma (default) / --exact
    int orbit_count = 0, frames = 1;
    bool cpu = false;                              // --cpu: ceres_render_cpu_f32 on the host cores
    int threads = 0;                               // --threads (0: the OpenMP default)
    std::string rays, hits_out, occluded_out;      // --rays: ray queries instead of a picture
    bool coherent = false;                         // --coherent: the plain ray query through ceres_trace_rays_coherent
    int all_hits = -1;                             // --all-hits K: the all-hits query, K records per ray (0: counts only)
    std::string counts_out;                        // ... its per-ray hit counts (uint32)
    std::string lists_out, offsets_out;            // --hit-lists-out / --offsets-out: the complete hit lists (CSR)
    bool lists() const { return !lists_out.empty() || !offsets_out.empty(); }
    std::string pixels_out, rgb8_out, status_out;  // ... and any of these: the shaded query
    bool shaded() const { return !pixels_out.empty() || !rgb8_out.empty() || !status_out.empty(); }
    std::vector<unsigned char> ray_bytes;          // the --rays file: raw ray32 (--double: ray64) records
    std::string points, nearest_out;               // --points / --nearest-out: the closest-point query
    std::vector<unsigned char> point_bytes;        // the --points file: raw point16 records
};

int usage() {
    std::fprintf(stderr,
                 "usage: render <obj> [--eye x y z] [--dir x y z] [--up x y z] [--fov deg] [--sun x y z]\n"
                 "              [--rotate x|y|z deg] [--size W H] [-o out.ppm] [--primary-only] [--proc N]\n"
                 "              [--device D] [--bench reps] [--json] [--orbit ax ay az step_deg count] [--frames N]\n"
                 "              [--gpu-bvh] [--double] [--gpus N] [--row-block R] [--robust] [--qbvh] [--exact|--fma]\n"
                 "              [--cpu [--threads T]] [--refit B.obj [--rebuild-above R]]\n"
                 "       render <obj> [--rotate x|y|z deg] --rays FILE --hits-out FILE [--occluded-out FILE] [--robust] [--coherent]\n"
                 "              [--exact|--fma] [--cpu [--threads T]] [--device D] [--json] [--double]\n"
                 "       render <obj> [--rotate x|y|z deg] --rays FILE --sun x y z --pixels-out FILE [--rgb8-out FILE]\n"
                 "              [--status-out FILE] [--hits-out FILE] [--robust] [--exact|--fma] [--cpu [--threads T]]\n"
                 "              [--device D] [--json] [--double]\n"
                 "       render <obj> [--rotate x|y|z deg] --rays FILE --all-hits K [--hits-out FILE] [--counts-out FILE]\n"
                 "              [--robust] [--exact|--fma] [--cpu [--threads T]] [--device D] [--json]\n"
                 "       render <obj> [--rotate x|y|z deg] --rays FILE --hit-lists-out FILE --offsets-out FILE [--robust]\n"
                 "              [--exact|--fma] [--cpu [--threads T]] [--device D] [--json]\n"
                 "       render <obj> [--rotate x|y|z deg] --points FILE --nearest-out FILE [--exact|--fma] [--cpu [--threads T]]\n"
                 "              [--device D] [--json]\n");
    return 2;
}

bool parse(int argc, char** argv, Opts& o) {
    // one number into both precisions; the whole string must convert
    auto num = [](const char* s, float* f, double* d) {
        char* e1; char* e2;
        *f = std::strtof(s, &e1);
        *d = std::strtod(s, &e2);
        return *e1 == '\0' && *e2 == '\0';
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto have = [&](int n) { return i + n < argc; };
        auto vec = [&](float* v, double* w) {
            if (!have(3)) return false;
            bool ok = num(argv[i + 1], v, w) && num(argv[i + 2], v + 1, w + 1) && num(argv[i + 3], v + 2, w + 2);
            i += 3;
            return ok;
        };
        if (a == "--eye") { if (!vec(o.f.eye, o.d.eye)) return false; }
        else if (a == "--dir") { if (!vec(o.f.dir, o.d.dir)) return false; }
        else if (a == "--up") { if (!vec(o.f.up, o.d.up)) return false; }
        else if (a == "--sun") { if (!vec(o.f.sun, o.d.sun)) return false; }
        else if (a == "--fov") { if (!have(1) || !num(argv[++i], &o.f.fov, &o.d.fov)) return false; }
        else if (a == "--rotate") {
            if (!have(2)) return false;
            const char c = argv[i + 1][0];
            o.rot_axis = c == 'x' ? 0 : c == 'y' ? 1 : c == 'z' ? 2 : -2;
            if (o.rot_axis == -2 || argv[i + 1][1] != '\0' || !num(argv[i + 2], &o.f.rot_deg, &o.d.rot_deg)) return false;
            i += 2;
        } else if (a == "--size") {
            if (!have(2)) return false;
            o.W = std::strtoul(argv[i + 1], nullptr, 10); o.H = std::strtoul(argv[i + 2], nullptr, 10); i += 2;
            if (!o.W || !o.H) return false;
        } else if (a == "-o" || a == "--out") { if (!have(1)) return false; o.out = argv[++i]; }
        else if (a == "--primary-only") o.mode = (o.mode & CERES_MODE_ROBUST) | CERES_MODE_PRIMARY;
        else if (a == "--robust") o.mode |= CERES_MODE_ROBUST;             // RobustNodeIntersector traversal
        else if (a == "--qbvh") o.mode |= CERES_MODE_QBVH4;                // compressed shadow BVH4 (not exact)
        else if (a == "--exact") o.arith = CERES_ARITH_EXACT;              // the -ffp-contract=off reference
        else if (a == "--fma") o.arith = CERES_ARITH_FMA;                  // the reference's CMake build
        else if (a == "--proc") { if (!have(1)) return false; o.proc = std::atoi(argv[++i]); }
        else if (a == "--device") { if (!have(1)) return false; o.device = std::atoi(argv[++i]); }
        else if (a == "--gpus") { if (!have(1)) return false; o.gpus = std::atoi(argv[++i]); if (o.gpus < 1) return false; }
        else if (a == "--row-block") { if (!have(1)) return false; o.row_block = std::atoi(argv[++i]); if (o.row_block < 1) return false; }
        else if (a == "--bench") { if (!have(1)) return false; o.bench = std::atoi(argv[++i]); }
        else if (a == "--json") o.json = true;
        else if (a == "--rays") { if (!have(1)) return false; o.rays = argv[++i]; }
        else if (a == "--hits-out") { if (!have(1)) return false; o.hits_out = argv[++i]; }
        else if (a == "--occluded-out") { if (!have(1)) return false; o.occluded_out = argv[++i]; }
        else if (a == "--coherent") o.coherent = true;
        else if (a == "--points") { if (!have(1)) return false; o.points = argv[++i]; }
        else if (a == "--nearest-out") { if (!have(1)) return false; o.nearest_out = argv[++i]; }
        else if (a == "--all-hits") {
            if (!have(1)) return false;
            char* end = nullptr;
            const long k = std::strtol(argv[++i], &end, 10);
            if (!*argv[i] || *end || k < 0 || k > 1000000) return false;
            o.all_hits = int(k);
        }
        else if (a == "--counts-out") { if (!have(1)) return false; o.counts_out = argv[++i]; }
        else if (a == "--hit-lists-out") { if (!have(1)) return false; o.lists_out = argv[++i]; }
        else if (a == "--offsets-out") { if (!have(1)) return false; o.offsets_out = argv[++i]; }
        else if (a == "--pixels-out") { if (!have(1)) return false; o.pixels_out = argv[++i]; }
        else if (a == "--rgb8-out") { if (!have(1)) return false; o.rgb8_out = argv[++i]; }
        else if (a == "--status-out") { if (!have(1)) return false; o.status_out = argv[++i]; }
        else if (a == "--refit") { if (!have(1)) return false; o.refit = argv[++i]; }
        else if (a == "--rebuild-above") {
            if (!have(1)) return false;
            char* e;
            o.rebuild_above = std::strtod(argv[++i], &e);
            if (*e != '\0' || e == argv[i]) return false;
            o.rebuild = true;
        }
        else if (a == "--cpu") o.cpu = true;
        else if (a == "--threads") { if (!have(1)) return false; o.threads = std::atoi(argv[++i]); if (o.threads < 0) return false; }
        else if (a == "--gpu-bvh") o.gpu_bvh = true;
        else if (a == "--double" || a == "-d") o.f64 = true;                   // anim.cpp:146-147
        else if (a == "--orbit") {
            if (!vec(o.f.orbit_axis, o.d.orbit_axis) || !have(2) || !num(argv[i + 1], &o.f.orbit_step, &o.d.orbit_step)) return false;
            o.orbit_count = std::atoi(argv[i + 2]); i += 2;
            if (o.orbit_count < 0) return false;
        } else if (a == "--frames") { if (!have(1)) return false; o.frames = std::atoi(argv[++i]); if (o.frames < 1) return false; }
        else if (a == "-h" || a == "--help") return false;
        else if (!a.empty() && a[0] == '-' && a.size() > 1 && !std::isdigit((unsigned char)a[1])) { std::fprintf(stderr, "unknown flag %s\n", a.c_str()); return false; }
        else if (o.obj.empty()) o.obj = a;
        else return false;
    }
    return !o.obj.empty() || o.proc > 0;
}

// The C ABI per precision (render<float> / render<double>).
template <class S> struct Api;
template <> struct Api<float> {
    using Node = uint32_t;
    static int load(const char* p, float** t, float** n, size_t* c, int ar) { return ceres_obj_load_arith(p, t, n, c, ar); }
    static int proc(int k, float** t, float** n, size_t* c, int ar) { return ceres_proc_mesh_arith(k, t, n, c, ar); }
    static int rotate(float* t, size_t c, int ax, float deg, int ar) { return ceres_rotate_triangles_arith(t, c, ax, deg, ar); }
    static int bvh(const float* t, size_t c, Node** nodes, size_t* m, uint64_t** prim, bool gpu, int dev, int ar) {
        return gpu ? ceres_bvh_build_gpu_arith(t, c, nodes, m, prim, dev, ar) : ceres_bvh_build_arith(t, c, nodes, m, prim, ar);
    }
    static ceres_scene* scene(const float* t, size_t c, const float* n, const Node* nodes, size_t m, const uint64_t* prim, int dev) {
        return ceres_scene_create(t, c, n, nodes, m, prim, dev, 0);
    }
    static int orbit(const Num<float>& v, size_t W, size_t H, uint32_t k, float* b, float* s, int ar) {
        return ceres_orbit_cameras_arith(v.eye, v.dir, v.up, v.sun, v.fov, W, H, v.orbit_axis, v.orbit_step, k, 0, b, s,
                                         nullptr, ar);
    }
    static int render(ceres_scene* sc, const float* b, const float* s, int mode, uint8_t* rgb, size_t W, size_t H, ceres_stats* st) {
        return ceres_render_f32(sc, b, s, mode, nullptr, rgb, W, H, st);
    }
    static int render_multi(ceres_scene* const* sc, uint32_t n, uint32_t rb, const float* b, const float* s, int mode,
                            uint8_t* rgb, size_t W, size_t H, ceres_stats* st) {
        return ceres_render_multi_f32(sc, n, rb, b, s, mode, nullptr, rgb, W, H, st);
    }
    static ceres_cpu_scene* cpu_scene(const float* t, size_t c, const float* n, const Node* nodes, size_t m, const uint64_t* prim) {
        return ceres_cpu_scene_create(t, c, n, nodes, m, prim);
    }
    static int render_cpu(const ceres_cpu_scene* cs, const float* b, const float* s, int mode, uint8_t* rgb, size_t W, size_t H,
                          ceres_stats* st, int threads) {
        return ceres_render_cpu_f32(cs, b, s, mode, nullptr, rgb, W, H, st, threads);
    }
    static int refit(ceres_scene* sc, const float* t, size_t c, const float* n) { return ceres_scene_refit(sc, t, c, n); }
    static int refit_cpu(ceres_cpu_scene* cs, const float* t, size_t c, const float* n) { return ceres_cpu_scene_refit(cs, t, c, n); }
    static int update(ceres_scene* sc, const float* t, size_t c, const float* n, int ar, double r, ceres_update_info* u) {
        return ceres_scene_update(sc, t, c, n, ar, r, u);
    }
    static int update_cpu(ceres_cpu_scene* cs, const float* t, size_t c, const float* n, int ar, double r, ceres_update_info* u) {
        return ceres_cpu_scene_update(cs, t, c, n, ar, r, u);
    }
    static constexpr size_t ray_bytes = 32, hit_bytes = 16;           // ray32 / hit16
    static int trace(ceres_scene* sc, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
        return ceres_trace_rays(sc, r, n, mode, h, oc, st);
    }
    static int trace_coherent(ceres_scene* sc, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
        return ceres_trace_rays_coherent(sc, r, n, mode, h, oc, st);
    }
    static int trace_cpu(const ceres_cpu_scene* cs, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st,
                         int threads) {
        return ceres_trace_rays_cpu(cs, r, n, mode, h, oc, st, threads);
    }
    static int shade(ceres_scene* sc, const void* r, size_t n, const float* sun, int mode, float* px, uint8_t* q, void* h,
                     uint8_t* s, ceres_stats* st) {
        return ceres_shade_rays(sc, r, n, sun, mode, px, q, h, s, st);
    }
    static int shade_cpu(const ceres_cpu_scene* cs, const void* r, size_t n, const float* sun, int mode, float* px, uint8_t* q,
                         void* h, uint8_t* s, ceres_stats* st, int threads) {
        return ceres_shade_rays_cpu(cs, r, n, sun, mode, px, q, h, s, st, threads);
    }
};
template <> struct Api<double> {
    using Node = uint64_t;
    // render<double> in either arithmetic (--fma: anim.cpp -d as the reference's CMake build compiles it)
    static int load(const char* p, double** t, double** n, size_t* c, int ar) { return ceres_obj_load_f64_arith(p, t, n, c, ar); }
    static int proc(int k, double** t, double** n, size_t* c, int ar) { return ceres_proc_mesh_f64_arith(k, t, n, c, ar); }
    static int rotate(double* t, size_t c, int ax, double deg, int ar) { return ceres_rotate_triangles_f64_arith(t, c, ax, deg, ar); }
    static int bvh(const double* t, size_t c, Node** nodes, size_t* m, uint64_t** prim, bool gpu, int dev, int ar) {
        return gpu ? ceres_bvh_build_f64_gpu_arith(t, c, nodes, m, prim, dev, ar) : ceres_bvh_build_f64_arith(t, c, nodes, m, prim, ar);
    }
    static ceres_scene* scene(const double* t, size_t c, const double* n, const Node* nodes, size_t m, const uint64_t* prim, int dev) {
        return ceres_scene_create_f64(t, c, n, nodes, m, prim, dev, 0);
    }
    static int orbit(const Num<double>& v, size_t W, size_t H, uint32_t k, double* b, double* s, int ar) {
        return ceres_orbit_cameras_f64_arith(v.eye, v.dir, v.up, v.sun, v.fov, W, H, v.orbit_axis, v.orbit_step, k, 0, b, s,
                                             nullptr, ar);
    }
    static int render(ceres_scene* sc, const double* b, const double* s, int mode, uint8_t* rgb, size_t W, size_t H, ceres_stats* st) {
        return ceres_render_f64(sc, b, s, mode, nullptr, rgb, W, H, st);
    }
    static int render_multi(ceres_scene* const*, uint32_t, uint32_t, const double*, const double*, int, uint8_t*, size_t,
                            size_t, ceres_stats*) {
        std::fprintf(stderr, "error: --gpus > 1 renders single precision only\n");
        return CERES_EUNSUPPORTED;
    }
    static ceres_cpu_scene* cpu_scene(const double* t, size_t c, const double* n, const Node* nodes, size_t m,
                                      const uint64_t* prim) {
        return ceres_cpu_scene_create_f64(t, c, n, nodes, m, prim);
    }
    static int render_cpu(const ceres_cpu_scene* cs, const double* b, const double* s, int mode, uint8_t* rgb, size_t W,
                          size_t H, ceres_stats* st, int threads) {
        return ceres_render_cpu_f64(cs, b, s, mode, nullptr, rgb, W, H, st, threads);
    }
    static int refit(ceres_scene* sc, const double* t, size_t c, const double* n) { return ceres_scene_refit_f64(sc, t, c, n); }
    static int refit_cpu(ceres_cpu_scene* cs, const double* t, size_t c, const double* n) { return ceres_cpu_scene_refit_f64(cs, t, c, n); }
    // the in-place rebuild of a double GPU scene is not implemented: the library refuses it before it reads the arrays
    static int update(ceres_scene* sc, const double* t, size_t c, const double* n, int ar, double r, ceres_update_info* u) {
        return ceres_scene_update(sc, reinterpret_cast<const float*>(t), c, reinterpret_cast<const float*>(n), ar, r, u);
    }
    static int update_cpu(ceres_cpu_scene* cs, const double* t, size_t c, const double* n, int ar, double r, ceres_update_info* u) {
        return ceres_cpu_scene_update_f64(cs, t, c, n, ar, r, u);
    }
    static constexpr size_t ray_bytes = 64, hit_bytes = 32;           // ray64 / hit32
    static int trace(ceres_scene* sc, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
        return ceres_trace_rays_f64(sc, r, n, mode, h, oc, st);
    }
    static int trace_coherent(ceres_scene* sc, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
        return ceres_trace_rays_coherent_f64(sc, r, n, mode, h, oc, st);
    }
    static int trace_cpu(const ceres_cpu_scene* cs, const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st,
                         int threads) {
        return ceres_trace_rays_cpu_f64(cs, r, n, mode, h, oc, st, threads);
    }
    static int shade(ceres_scene* sc, const void* r, size_t n, const double* sun, int mode, double* px, uint8_t* q, void* h,
                     uint8_t* s, ceres_stats* st) {
        return ceres_shade_rays_f64(sc, r, n, sun, mode, px, q, h, s, st);
    }
    static int shade_cpu(const ceres_cpu_scene* cs, const void* r, size_t n, const double* sun, int mode, double* px, uint8_t* q,
                         void* h, uint8_t* s, ceres_stats* st, int threads) {
        return ceres_shade_rays_cpu_f64(cs, r, n, sun, mode, px, q, h, s, st, threads);
    }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class S, class Render>
int frames_loop(const Opts& o, const Num<S>& v, Render&& render, const char* where);

// --rays: the file's ray32 / ray64 records through `trace` (ceres_trace_rays / ceres_trace_rays_cpu or
// their _f64 siblings), the answers written as raw hit16 / hit32 records (--hits-out) and raw 0 / 1
// bytes (--occluded-out).
template <class S, class Trace>
int rays_run(const Opts& o, Trace&& trace, const char* where) {
    const size_t n = o.ray_bytes.size() / Api<S>::ray_bytes;
    std::vector<unsigned char> hits(o.hits_out.empty() ? 0 : Api<S>::hit_bytes * n), occ(o.occluded_out.empty() ? 0 : n);
    ceres_stats st{};
    std::printf("Tracing %zu ray(s) on the %s...\n", n, where);
    const int mode = o.mode & (CERES_MODE_ROBUST | CERES_MODE_FMA);
    if (trace(o.ray_bytes.data(), n, mode, o.hits_out.empty() ? nullptr : hits.data(), o.occluded_out.empty() ? nullptr : occ.data(),
              &st) != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        return 1;
    }
    auto write = [](const std::string& path, const std::vector<unsigned char>& b) {
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", path.c_str()); return false; }
        const bool ok = std::fwrite(b.data(), 1, b.size(), f) == b.size();
        return (std::fclose(f) == 0) && ok;
    };
    if (!o.hits_out.empty() && !write(o.hits_out, hits)) return 1;
    if (!o.occluded_out.empty() && !write(o.occluded_out, occ)) return 1;
    std::printf("Rays: %llu\tHits: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits);
    if (o.json) std::printf("{\"rays\": %llu, \"hits\": %llu, \"ms\": %.4f}\n", (unsigned long long)st.rays,
                            (unsigned long long)st.hits, st.ms);
    return 0;
}

// --points with --nearest-out: the file's point16 records through `closest` (ceres_closest_points /
// ceres_closest_points_cpu), the answers written as raw near16 records.
template <class Closest>
int nearest_run(const Opts& o, Closest&& closest, const char* where) {
    const size_t n = o.point_bytes.size() / 16;
    std::vector<unsigned char> near(16 * n + 16);                    // (never empty: n = 0 still has an output pointer)
    ceres_stats st{};
    std::printf("Finding the closest surface point of %zu point(s) on the %s...\n", n, where);
    if (closest(o.point_bytes.data(), n, near.data(), &st) != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        return 1;
    }
    FILE* f = std::fopen(o.nearest_out.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "error: cannot write %s\n", o.nearest_out.c_str()); return 1; }
    const bool ok = std::fwrite(near.data(), 1, 16 * n, f) == 16 * n;
    if (std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "error: cannot write %s\n", o.nearest_out.c_str()); return 1; }
    std::printf("Points: %llu\tFound: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits);
    if (o.json) std::printf("{\"points\": %llu, \"found\": %llu, \"ms\": %.4f}\n", (unsigned long long)st.rays,
                            (unsigned long long)st.hits, st.ms);
    return 0;
}

// --rays with --all-hits K: the file's ray32 records through `trace_all` (ceres_trace_rays_all /
// ceres_trace_rays_all_cpu), each ray's K hit16 records written ray after ray (--hits-out) and the
// per-ray sizes of the hit sets as raw uint32 (--counts-out).  K = 0: counts only.
template <class TraceAll>
int all_hits_run(const Opts& o, TraceAll&& trace_all, const char* where) {
    const size_t n = o.ray_bytes.size() / 32;
    const uint32_t K = uint32_t(o.all_hits);
    std::vector<unsigned char> hits(o.hits_out.empty() ? 0 : 16 * n * size_t(K));
    std::vector<uint32_t> counts(o.counts_out.empty() ? 0 : n);
    ceres_stats st{};
    std::printf("Tracing %zu ray(s) for all hits on the %s...\n", n, where);
    const int mode = o.mode & (CERES_MODE_ROBUST | CERES_MODE_FMA);
    // an empty vector's data() may be NULL: a zero-ray file still names its outputs
    alignas(16) static unsigned char none[16];
    void* hp = o.hits_out.empty() ? nullptr : (hits.empty() ? static_cast<void*>(none) : hits.data());
    uint32_t* cp = o.counts_out.empty() ? nullptr : (counts.empty() ? reinterpret_cast<uint32_t*>(none) : counts.data());
    if (trace_all(o.ray_bytes.data(), n, mode, K, cp, hp, &st) != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        return 1;
    }
    auto write = [](const std::string& path, const void* b, size_t bytes) {
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", path.c_str()); return false; }
        const bool ok = std::fwrite(b, 1, bytes, f) == bytes;
        return (std::fclose(f) == 0) && ok;
    };
    if (!o.hits_out.empty() && !write(o.hits_out, hits.data(), hits.size())) return 1;
    if (!o.counts_out.empty() && !write(o.counts_out, counts.data(), counts.size() * 4)) return 1;
    std::printf("Rays: %llu\tHits: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits);
    if (o.json) std::printf("{\"rays\": %llu, \"hits\": %llu, \"max_hits\": %u, \"ms\": %.4f}\n", (unsigned long long)st.rays,
                            (unsigned long long)st.hits, K, st.ms);
    return 0;
}

// --rays with --hit-lists-out and --offsets-out: the file's ray32 records through `trace_lists`
// (ceres_trace_rays_lists / ceres_trace_rays_lists_cpu): every hit of every ray as hit16 records, ray
// after ray without padding, and the n + 1 uint64 offsets of the rays' segments.  The call is made
// twice: without a buffer for the total, then with one of that size.
template <class TraceLists>
int lists_run(const Opts& o, TraceLists&& trace_lists, const char* where) {
    const size_t n = o.ray_bytes.size() / 32;
    std::vector<uint64_t> offsets(n + 1);
    uint64_t total = 0;
    ceres_stats st{};
    std::printf("Tracing %zu ray(s) for complete hit lists on the %s...\n", n, where);
    const int mode = o.mode & (CERES_MODE_ROBUST | CERES_MODE_FMA);
    int rc = trace_lists(o.ray_bytes.data(), n, mode, offsets.data(), nullptr, 0, &total, &st);
    std::vector<unsigned char> hits;
    if (rc == CERES_ENOMEM && total) {
        hits.resize(size_t(total) * 16);
        rc = trace_lists(o.ray_bytes.data(), n, mode, offsets.data(), hits.data(), total, &total, &st);
    }
    if (rc != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        return 1;
    }
    auto write = [](const std::string& path, const void* b, size_t bytes) {
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", path.c_str()); return false; }
        const bool ok = std::fwrite(b, 1, bytes, f) == bytes;
        return (std::fclose(f) == 0) && ok;
    };
    if (!write(o.lists_out, hits.data(), hits.size()) || !write(o.offsets_out, offsets.data(), offsets.size() * 8)) return 1;
    std::printf("Rays: %llu\tHits: %llu\tRecords: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits,
                (unsigned long long)total);
    if (o.json) std::printf("{\"rays\": %llu, \"hits\": %llu, \"records\": %llu, \"ms\": %.4f}\n", (unsigned long long)st.rays,
                            (unsigned long long)st.hits, (unsigned long long)total, st.ms);
    return 0;
}

// --rays with --pixels-out / --rgb8-out / --status-out: the file's ray32 / ray64 records through `shade`
// (ceres_shade_rays / ceres_shade_rays_cpu or their _f64 siblings), the outputs written as raw arrays in
// ray order (pixels: 3 floats, with --double 3 doubles, per ray).
template <class S, class Shade>
int shade_run(const Opts& o, Shade&& shade, const char* where) {
    const size_t n = o.ray_bytes.size() / Api<S>::ray_bytes;
    std::vector<S> px(o.pixels_out.empty() ? 0 : 3 * n);
    std::vector<unsigned char> rgb(o.rgb8_out.empty() ? 0 : 3 * n), hits(o.hits_out.empty() ? 0 : Api<S>::hit_bytes * n),
        status(o.status_out.empty() ? 0 : n);
    ceres_stats st{};
    std::printf("Shading %zu ray(s) on the %s...\n", n, where);
    const int mode = o.mode & (CERES_MODE_ROBUST | CERES_MODE_FMA);
    if (shade(o.ray_bytes.data(), n, mode, o.pixels_out.empty() ? nullptr : px.data(), o.rgb8_out.empty() ? nullptr : rgb.data(),
              o.hits_out.empty() ? nullptr : hits.data(), o.status_out.empty() ? nullptr : status.data(), &st) != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        return 1;
    }
    auto write = [](const std::string& path, const void* b, size_t bytes) {
        if (path.empty()) return true;
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "error: cannot write %s\n", path.c_str()); return false; }
        const bool ok = std::fwrite(b, 1, bytes, f) == bytes;
        return (std::fclose(f) == 0) && ok;
    };
    if (!write(o.pixels_out, px.data(), sizeof(S) * px.size()) || !write(o.rgb8_out, rgb.data(), rgb.size()) ||
        !write(o.hits_out, hits.data(), hits.size()) || !write(o.status_out, status.data(), status.size()))
        return 1;
    std::printf("Rays: %llu\tHits: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits);
    if (o.json) std::printf("{\"rays\": %llu, \"hits\": %llu, \"primary_rays\": %llu, \"shadow_rays\": %llu, \"ms\": %.4f}\n",
                            (unsigned long long)st.rays, (unsigned long long)st.hits, (unsigned long long)st.primary_rays,
                            (unsigned long long)st.shadow_rays, st.ms);
    return 0;
}

// --refit: B's triangles and normals, loaded and rotated like the first OBJ, handed to `refit` (one
// call per scene copy); 0 on success, 1 after printing the error.
// --rebuild-above: one line per updated scene
int report_update(int rc, const ceres_update_info& u) {
    if (rc == CERES_OK)
        std::printf("SAH cost: %.6f\tbuilt: %.6f\tratio: %.6f\t%s\n", u.cost, u.built_cost, u.cost / u.built_cost,
                    u.rebuilt ? "rebuilt" : "kept");
    return rc;
}

template <class S, class Refit>
int refit_run(const Opts& o, const Num<S>& v, size_t n_tri, Refit&& refit) {
    using A = Api<S>;
    S* tri = nullptr; S* norm = nullptr; size_t n = 0;
    if (A::load(o.refit.c_str(), &tri, &norm, &n, o.arith) != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
    int rc = 0;
    if (n != n_tri) {
        std::fprintf(stderr, "error: --refit %s has %zu triangle(s), the scene has %zu: a refit keeps the face count\n",
                     o.refit.c_str(), n, n_tri);
        rc = 1;
    } else {
        if (o.rot_axis >= 0) A::rotate(tri, n, o.rot_axis, v.rot_deg, o.arith);
        std::printf(o.rebuild ? "Updating the BVH for %s...\n" : "Refitting the BVH to %s...\n", o.refit.c_str());
        if (refit(tri, n, norm) != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); rc = 1; }
    }
    ceres_free(tri); ceres_free(norm);
    return rc;
}

template <class S>
int run(const Opts& o, const Num<S>& v) {
    using A = Api<S>;
    S* tri = nullptr; S* norm = nullptr; size_t n_tri = 0;
    const int rc_load = o.proc ? A::proc(o.proc, &tri, &norm, &n_tri, o.arith) : A::load(o.obj.c_str(), &tri, &norm, &n_tri, o.arith);
    if (rc_load != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
    if (n_tri == 0) { std::fprintf(stderr, "The given scene is empty or cannot be loaded\n"); return 1; }   // static.cpp:77-80
    if (o.rot_axis >= 0) A::rotate(tri, n_tri, o.rot_axis, v.rot_deg, o.arith);

    std::printf("Building BVH ( using BinnedSahBuilder%s )...\n", o.gpu_bvh ? " on the GPU" : "");
    const double t0 = now_s();
    typename A::Node* nodes = nullptr; uint64_t* prim = nullptr; size_t n_nodes = 0;
    const int rc_bvh = A::bvh(tri, n_tri, &nodes, &n_nodes, &prim, o.gpu_bvh, o.device, o.arith);
    if (rc_bvh != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
    std::printf("%g\n", now_s() - t0);
    std::printf("BVH of %zu node(s) and %zu reference(s)\n", n_nodes, n_tri);

    if (o.cpu) {
        ceres_cpu_scene* cs = A::cpu_scene(tri, n_tri, norm, nodes, n_nodes, prim);
        ceres_free(nodes); ceres_free(prim); ceres_free(tri); ceres_free(norm);
        if (!cs) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
        if (!o.refit.empty() && refit_run<S>(o, v, n_tri, [&](const S* t, size_t n, const S* nn) {
                ceres_update_info u{};
                return o.rebuild ? report_update(A::update_cpu(cs, t, n, nn, o.arith, o.rebuild_above, &u), u) : A::refit_cpu(cs, t, n, nn);
            })) {
            ceres_cpu_scene_destroy(cs);
            return 1;
        }
        if (!o.points.empty()) {                                       // a double scene: the library's refusal
            const int rc = nearest_run(o, [&](const void* p, size_t n, void* out, ceres_stats* st) {
                return ceres_closest_points_cpu(cs, p, n, out, st, o.threads);
            }, "CPU");
            ceres_cpu_scene_destroy(cs);
            return rc;
        }
        if (!o.rays.empty() && o.shaded()) {
            const int rc = shade_run<S>(o, [&](const void* r, size_t n, int mode, S* px, uint8_t* q, void* h, uint8_t* s, ceres_stats* st) {
                return A::shade_cpu(cs, r, n, v.sun, mode, px, q, h, s, st, o.threads);
            }, "CPU");
            ceres_cpu_scene_destroy(cs);
            return rc;
        }
        if (!o.rays.empty() && o.lists()) {                            // a double scene: the library's refusal
            const int rc = lists_run(o, [&](const void* r, size_t n, int mode, uint64_t* of, void* h, uint64_t cap, uint64_t* tot,
                                            ceres_stats* st) {
                return ceres_trace_rays_lists_cpu(cs, r, n, mode, of, h, cap, tot, st, o.threads);
            }, "CPU");
            ceres_cpu_scene_destroy(cs);
            return rc;
        }
        if (!o.rays.empty() && o.all_hits >= 0) {                      // a double scene: the library's refusal
            const int rc = all_hits_run(o, [&](const void* r, size_t n, int mode, uint32_t k, uint32_t* c, void* h, ceres_stats* st) {
                return ceres_trace_rays_all_cpu(cs, r, n, mode, k, c, h, st, o.threads);
            }, "CPU");
            ceres_cpu_scene_destroy(cs);
            return rc;
        }
        if (!o.rays.empty()) {
            const int rc = rays_run<S>(o, [&](const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
                return A::trace_cpu(cs, r, n, mode, h, oc, st, o.threads);
            }, "CPU");
            ceres_cpu_scene_destroy(cs);
            return rc;
        }
        const int rc = frames_loop(o, v, [&](const S* basis, const S* sun, uint8_t* rgb, ceres_stats* st) {
            return A::render_cpu(cs, basis, sun, o.mode, rgb, o.W, o.H, st, o.threads);
        }, "CPU");
        ceres_cpu_scene_destroy(cs);
        return rc;
    }
    ceres_scene* scene = A::scene(tri, n_tri, norm, nodes, n_nodes, prim, o.device);
    // --gpus N: one scene copy per further rank, on the next devices (mod the device count)
    std::vector<ceres_scene*> ranks(1, scene);
    if (scene && o.gpus > 1) {
        const int ndev = ceres_device_count();
        for (int r = 1; r < o.gpus && ndev > 0; ++r) {
            ceres_scene* sr = A::scene(tri, n_tri, norm, nodes, n_nodes, prim, (o.device + r) % ndev);
            if (!sr) break;
            ranks.push_back(sr);
        }
    }
    ceres_free(nodes); ceres_free(prim); ceres_free(tri); ceres_free(norm);
    auto destroy = [&] { for (auto* sr : ranks) ceres_scene_destroy(sr); };
    if (!scene || int(ranks.size()) != o.gpus) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error());
        destroy();
        return 1;
    }
    if (!o.refit.empty() && refit_run<S>(o, v, n_tri, [&](const S* t, size_t n, const S* nn) {
            for (auto* sr : ranks) {
                ceres_update_info u{};
                if (int rc = o.rebuild ? report_update(A::update(sr, t, n, nn, o.arith, o.rebuild_above, &u), u) : A::refit(sr, t, n, nn))
                    return rc;
            }
            return int(CERES_OK);
        })) {
        destroy();
        return 1;
    }
    if (!o.points.empty()) {                                           // a double scene: the library's refusal
        const int rc = nearest_run(o, [&](const void* p, size_t n, void* out, ceres_stats* st) {
            return ceres_closest_points(scene, p, n, out, st);
        }, "HIP device");
        destroy();
        return rc;
    }
    if (!o.rays.empty() && o.shaded()) {
        const int rc = shade_run<S>(o, [&](const void* r, size_t n, int mode, S* px, uint8_t* q, void* h, uint8_t* s, ceres_stats* st) {
            return A::shade(scene, r, n, v.sun, mode, px, q, h, s, st);
        }, "HIP device");
        destroy();
        return rc;
    }
    if (!o.rays.empty() && o.lists()) {                                // a double scene: the library's refusal
        const int rc = lists_run(o, [&](const void* r, size_t n, int mode, uint64_t* of, void* h, uint64_t cap, uint64_t* tot,
                                        ceres_stats* st) {
            return ceres_trace_rays_lists(scene, r, n, mode, of, h, cap, tot, st);
        }, "HIP device");
        destroy();
        return rc;
    }
    if (!o.rays.empty() && o.all_hits >= 0) {                          // a double scene: the library's refusal
        const int rc = all_hits_run(o, [&](const void* r, size_t n, int mode, uint32_t k, uint32_t* c, void* h, ceres_stats* st) {
            return ceres_trace_rays_all(scene, r, n, mode, k, c, h, st);
        }, "HIP device");
        destroy();
        return rc;
    }
    if (!o.rays.empty()) {
        const int rc = rays_run<S>(o, [&](const void* r, size_t n, int mode, void* h, uint8_t* oc, ceres_stats* st) {
            return o.coherent ? A::trace_coherent(scene, r, n, mode, h, oc, st) : A::trace(scene, r, n, mode, h, oc, st);
        }, "HIP device");
        destroy();
        return rc;
    }
    auto render = [&](const S* basis, const S* sun, uint8_t* rgb, ceres_stats* st) {
        return o.gpus > 1 ? A::render_multi(ranks.data(), uint32_t(o.gpus), uint32_t(o.row_block), basis, sun, o.mode, rgb,
                                            o.W, o.H, st)
                          : A::render(scene, basis, sun, o.mode, rgb, o.W, o.H, st);
    };
    const int rc = frames_loop(o, v, render, "HIP");
    destroy();
    return rc;
}

// The frame loop of static.cpp / anim.cpp (render :130 / :104-110, PPM :135-147, "Total Rays"
// anim.cpp:127) over `render`; `where` names the render path in the progress lines.
template <class S, class Render>
int frames_loop(const Opts& o, const Num<S>& v, Render&& render, const char* where) {
    using A = Api<S>;

    // frame poses: count + k orbit rotations for frame k (count = 0, frames = 1: the plain camera)
    const uint32_t n_pose = uint32_t(o.orbit_count + o.frames);
    std::vector<S> bases(12 * size_t(n_pose)), suns(3 * size_t(n_pose));
    if (A::orbit(v, o.W, o.H, n_pose, bases.data(), suns.data(), o.arith) != CERES_OK) {
        std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1;
    }
    std::vector<uint8_t> rgb(3 * o.W * o.H);
    ceres_stats st{};
    unsigned long long tot_rays = 0;
    std::vector<double> ms, e2e;
    for (int k = 0; k < o.frames; ++k) {
        const S* basis = bases.data() + 12 * size_t(o.orbit_count + k);
        const S* sun = suns.data() + 3 * size_t(o.orbit_count + k);
        if (o.cpu) std::printf("Rendering image %d (%zux%zu) on the %s%s...\n", k, o.W, o.H, where,
                               o.threads ? (" with " + std::to_string(o.threads) + " threads").c_str() : "");
        else if (o.gpus > 1) std::printf("Rendering image %d (%zux%zu) on %d %s ranks from device %d...\n", k, o.W, o.H, o.gpus, where, o.device);
        else std::printf("Rendering image %d (%zux%zu) on %s device %d...\n", k, o.W, o.H, where, o.device);
        const double t1 = now_s();
        int rc = render(basis, sun, rgb.data(), &st);
        const double t2 = now_s();
        if (rc != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
        std::printf("%g\n", t2 - t1);
        std::printf("Rays: %llu\tHits: %llu\n", (unsigned long long)st.rays, (unsigned long long)st.hits);   // anim.cpp:109
        tot_rays += st.rays;
        for (int r = 0; r < o.bench; ++r) {
            ceres_stats s2{};
            const double b1 = now_s();
            rc = render(basis, sun, rgb.data(), &s2);
            e2e.push_back((now_s() - b1) * 1e3);          // the whole call: launch + kernel + RGB8 copy to the host
            if (rc != CERES_OK) { std::fprintf(stderr, "error: %s\n", ceres_last_error()); return 1; }
            ms.push_back(s2.ms);
        }
        std::string path = o.out;
        if (o.frames > 1) {
            char suffix[16];
            std::snprintf(suffix, sizeof suffix, "_%03d", k);
            const size_t dot = path.rfind('.');
            const size_t slash = path.rfind('/');
            if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) path += suffix;
            else path.insert(dot, suffix);
        }
        if (FILE* f = std::fopen(path.c_str(), "wb")) {              // static.cpp:135-147
            std::fprintf(f, "P6 %zu %zu %d\n", o.W, o.H, 255);
            std::fwrite(rgb.data(), 1, rgb.size(), f);
            std::fclose(f);
        } else {
            std::fprintf(stderr, "error: cannot write %s\n", path.c_str());
            return 1;
        }
    }
    if (o.frames > 1) std::printf("Total Rays: %llu\n", tot_rays);   // anim.cpp:127
    if (o.json) {
        double med = 0, e2e_med = 0;
        if (!ms.empty()) { std::sort(ms.begin(), ms.end()); med = ms[ms.size() / 2]; }
        if (!e2e.empty()) { std::sort(e2e.begin(), e2e.end()); e2e_med = e2e[e2e.size() / 2]; }
        std::printf("{\"rays\": %llu, \"hits\": %llu, \"W\": %zu, \"H\": %zu, \"device_ms\": %.4f, \"bench_median_ms\": %.4f, "
                    "\"mrays_per_s\": %.3f, \"e2e_ms\": %.4f}\n",
                    (unsigned long long)st.rays, (unsigned long long)st.hits, o.W, o.H, st.ms, med,
                    med > 0 ? double(st.rays) / (med * 1e3) : 0.0, e2e_med);
    }
    if (o.json && o.cpu)                                              // the reference's Statistics, all rays
        std::printf("{\"node_pairs\": %llu, \"tri_tests\": %llu, \"primary_rays\": %llu, \"shadow_rays\": %llu}\n",
                    (unsigned long long)st.node_pairs, (unsigned long long)st.tri_tests,
                    (unsigned long long)st.primary_rays, (unsigned long long)st.shadow_rays);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Opts o;
    if (!parse(argc, argv, o)) return usage();
    if (o.arith == CERES_ARITH_FMA) o.mode |= CERES_MODE_FMA;
    if (o.rebuild && o.refit.empty()) { std::fprintf(stderr, "error: --rebuild-above R goes with --refit B.obj\n"); return 2; }
    if (!o.refit.empty() && o.proc) { std::fprintf(stderr, "error: --refit takes OBJ scenes (not with --proc)\n"); return 2; }
    if (o.cpu && (o.gpus > 1 || o.gpu_bvh || (o.mode & CERES_MODE_QBVH4))) {
        std::fprintf(stderr, "error: --cpu renders in one process on the host (not with --gpus, --gpu-bvh, --qbvh)\n");
        return 2;
    }
    if (!o.points.empty() || !o.nearest_out.empty()) {
        if (o.points.empty() || o.nearest_out.empty()) {
            std::fprintf(stderr, "error: the closest-point query takes --points FILE and --nearest-out FILE, both\n");
            return 2;
        }
        if (!o.rays.empty() || !o.hits_out.empty() || !o.occluded_out.empty() || o.shaded() || o.all_hits >= 0 || !o.counts_out.empty() ||
            o.lists() || o.coherent) {
            std::fprintf(stderr, "error: --points / --nearest-out do not go with --rays or its outputs\n");
            return 2;
        }
        if (o.gpus > 1 || (o.mode & (CERES_MODE_PRIMARY | CERES_MODE_QBVH4))) {
            std::fprintf(stderr, "error: --points runs on one device (not with --gpus, --primary-only, --qbvh)\n");
            return 2;
        }
        FILE* f = std::fopen(o.points.c_str(), "rb");
        if (!f) { std::fprintf(stderr, "error: cannot read %s\n", o.points.c_str()); return 1; }
        unsigned char buf[1 << 16];
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) o.point_bytes.insert(o.point_bytes.end(), buf, buf + k);
        std::fclose(f);
        if (o.point_bytes.size() % 16) {
            std::fprintf(stderr, "error: %s holds %zu bytes, not a whole number of 16-byte point records\n", o.points.c_str(),
                         o.point_bytes.size());
            return 2;
        }
    }
    if (o.shaded()) {
        if (o.rays.empty()) { std::fprintf(stderr, "error: --pixels-out / --rgb8-out / --status-out need --rays\n"); return 2; }
        if (!o.occluded_out.empty()) {
            std::fprintf(stderr, "error: --occluded-out is an output of the plain ray query (not with --pixels-out / --rgb8-out / --status-out)\n");
            return 2;
        }
    }
    if (o.all_hits >= 0) {
        if (o.rays.empty() || o.shaded() || !o.occluded_out.empty()) {
            std::fprintf(stderr, "error: --all-hits K goes with --rays, --hits-out and / or --counts-out (not with --occluded-out or the shaded outputs)\n");
            return 2;
        }
        if (o.hits_out.empty() && o.counts_out.empty()) { std::fprintf(stderr, "error: --all-hits needs --hits-out and / or --counts-out\n"); return 2; }
        if (o.all_hits == 0 && !o.hits_out.empty()) { std::fprintf(stderr, "error: --all-hits 0 is the count-only query (--counts-out alone)\n"); return 2; }
    } else if (!o.counts_out.empty()) {
        std::fprintf(stderr, "error: --counts-out needs --all-hits\n");
        return 2;
    }
    if (o.lists()) {
        if (o.lists_out.empty() || o.offsets_out.empty() || o.rays.empty()) {
            std::fprintf(stderr, "error: complete hit lists take --rays, --hit-lists-out and --offsets-out, all three\n");
            return 2;
        }
        if (o.all_hits >= 0 || !o.hits_out.empty() || !o.occluded_out.empty() || o.shaded()) {
            std::fprintf(stderr, "error: --hit-lists-out / --offsets-out do not go with --all-hits, --hits-out, --occluded-out or the shaded outputs\n");
            return 2;
        }
    }
    if (!o.rays.empty()) {
        if (!o.shaded() && o.all_hits < 0 && !o.lists() && o.hits_out.empty() && o.occluded_out.empty()) { std::fprintf(stderr, "error: --rays needs --hits-out and / or --occluded-out\n"); return 2; }
        if (o.gpus > 1 || (o.mode & (CERES_MODE_PRIMARY | CERES_MODE_QBVH4))) {
            std::fprintf(stderr, "error: --rays traces on one device (not with --gpus, --primary-only, --qbvh)\n");
            return 2;
        }
        FILE* f = std::fopen(o.rays.c_str(), "rb");
        if (!f) { std::fprintf(stderr, "error: cannot read %s\n", o.rays.c_str()); return 1; }
        unsigned char buf[1 << 16];
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) o.ray_bytes.insert(o.ray_bytes.end(), buf, buf + k);
        std::fclose(f);
        const size_t rec = o.f64 && o.all_hits < 0 && !o.lists() ? 64 : 32;   // ray64 / ray32 (the all-hits queries: ray32 only)
        if (o.ray_bytes.size() % rec) {
            std::fprintf(stderr, "error: %s holds %zu bytes, not a whole number of %zu-byte ray records%s\n", o.rays.c_str(),
                         o.ray_bytes.size(), rec, o.f64 ? " (--double reads ray64)" : "");
            return 2;
        }
    } else if (!o.hits_out.empty() || !o.occluded_out.empty()) {
        std::fprintf(stderr, "error: --hits-out / --occluded-out need --rays\n");
        return 2;
    }
    if (o.coherent && (o.rays.empty() || o.shaded() || o.all_hits >= 0 || o.lists() || o.cpu)) {
        std::fprintf(stderr, "error: --coherent goes with the plain ray query on the GPU (--rays with --hits-out / --occluded-out)\n");
        return 2;
    }
    return o.f64 ? run<double>(o, o.d) : run<float>(o, o.f);
}
