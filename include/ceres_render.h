/* ceres_render.h -- C ABI of the MI355X-native CERES hot path (libceres_hip.so).
 *
 * The reference has no C ABI, plugin registry or FFI: its hot path is the header-only
 * template `render()` (include/render.hpp:86-156 in iracigt/ceres-raytracer) plus the
 * host-side scene preparation its callers run first (static.cpp:76-107, anim.cpp:38-65).
 * Every entry point below replaces one of those reference interfaces; the reference
 * file:line is cited per function.  Plain pointers and sizes only -- no C++ or torch
 * types -- so it can be bound from C, C++, ctypes, cgo, JNI ...
 *
 * Data layouts (all little-endian, fp32 unless stated), identical to the reference's
 * in-memory structures so a caller can hand its own arrays over unchanged:
 *   tri48   n_tri  x {p0[3], e1[3], e2[3], n[3]}        = bvh::Triangle<float> (triangle.hpp:17-37)
 *   norm36  n_tri  x {n0[3], n1[3], n2[3]}              = std::array<Vector3,3> (obj_norms.hpp:113-115)
 *   nodes32 n_nodes x {bounds[6], u32 count, u32 first} = bvh::Bvh<float>::Node (bvh.hpp:25-30)
 *   prim64  n_tri  x u64                                = Bvh::primitive_indices (bvh.hpp:94)
 *   pixels  3*W*H  floats, row j = 0 at the BOTTOM       (render.hpp:107)
 *   rgb8    3*W*H  bytes = the P6 body, rows top-down, truncating quantiser (static.cpp:135-147)
 *
 * Errors: functions return 0 on success and a negative ceres_status on failure;
 * ceres_last_error() describes the last failure of the calling thread.  The product
 * path has NO CPU fallback: without a usable gfx950 device every render call fails.
 * Threading: a ceres_scene is not thread-safe; use one scene per thread (or lock).
 */
#ifndef CERES_RENDER_H
#define CERES_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CERES_OK = 0,
    CERES_EINVAL = -1,      /* bad argument (null pointer, zero size, malformed BVH) */
    CERES_EIO = -2,         /* file could not be read / malformed OBJ index (obj_norms.hpp:90) */
    CERES_ENOMEM = -3,      /* host or device allocation failed */
    CERES_EHIP = -4,        /* HIP runtime error (no device, launch failure, ...) */
    CERES_ESTACK = -5,      /* traversal stack overflow (single_ray_traverser.hpp:29 assert) */
    CERES_EUNSUPPORTED = -6
} ceres_status;

typedef enum {
    CERES_MODE_FULL = 0,     /* primary + shadow + smooth shading (render.hpp:104-153) */
    CERES_MODE_PRIMARY = 1,  /* primary rays only; pixel = |normalize(tri.n)| (render.hpp:123-125) */
    CERES_MODE_ROBUST = 0x10, /* OR-ed flag: traverse with the library's RobustNodeIntersector
                                (node_intersectors.hpp:54-79) instead of render()'s FastNodeIntersector;
                                float scenes only */
    CERES_MODE_QBVH4 = 0x20, /* OR-ed flag (full mode, float, not with ROBUST): shadow rays traverse
                                a COMPRESSED BVH4 -- 64-B nodes, child boxes quantised to 8 bits per
                                bound, rounded outwards -- instead of the exact 128-B one.  Not
                                bit-exact: a box can only grow, so every leaf the reference reaches
                                is still tested, but a grazing shadow ray may also meet a triangle
                                the reference's slab tests never reach (a lit pixel turns dark).
                                Held to the SURVEY section 7 budget (+-1 LSB, <= 1e-5 of pixels),
                                never the default (node_intersectors.hpp:35-47,83-103). */
    CERES_MODE_FMA = 0x40    /* OR-ed flag: the arithmetic of the reference as its own CMake build
                                compiles it (CMakeLists.txt:11-13, g++ -O3 -mavx2 -mfma, where GCC
                                contracts a*b+c into FMA): an explicit fmaf at exactly the sites GCC
                                fuses (primary direction render.hpp:111, Moller-Trumbore
                                triangle.hpp:98-109, hit point :129-133, normalize/cross/dot
                                vector.hpp:134-167, shading render.hpp:48-81; the list with the
                                compiler evidence is oracle/contraction_sites.txt).  Bit-identical to
                                _ref/ref_render (the reference-flag build) given a scene prepared with
                                CERES_ARITH_FMA; without it, bit-identical to the -ffp-contract=off
                                build.  Combines with ROBUST, QBVH4 and PRIMARY. */
} ceres_mode;

/* Arithmetic of the host scene preparation (the *_arith calls below): CERES_ARITH_EXACT is the
 * reference compiled without contraction, CERES_ARITH_FMA the reference's own CMake build (the
 * triangle normals cross(e1, e2), the rotation, the vertex-normal normalisation, the SAH costs,
 * the camera basis and the orbit Transform all contract there, so that build's scene differs
 * bit-wise from the exact one: pair it with CERES_MODE_FMA renders). */
#define CERES_ARITH_EXACT 0
#define CERES_ARITH_FMA   1

typedef struct ceres_scene ceres_scene;

/* Per-render counters.  rays/hits are exactly render()'s return pair (render.hpp:102,115,
 * 119,138,148,155) widened to 64 bit.  The traversal counters are filled only when the
 * scene was created with CERES_SCENE_STATS (they follow single_ray_traverser.hpp:132-135,
 * except that shadow rays stop at the first occluder -- any-hit, result-identical). */
typedef struct {
    uint64_t rays;            /* primary + shadow traversals */
    uint64_t hits;            /* primary hits + occluded shadow rays */
    uint64_t primary_rays, shadow_rays;
    uint64_t node_pairs;      /* traversal_steps, all rays */
    uint64_t tri_tests;       /* intersections, all rays */
    double   ms;              /* device time of the render (HIP events), host-buffer API only */
} ceres_stats;

/* Row partition across ranks; world = 1 renders the whole frame.
 * bands = 0: rows are dealt in blocks of `row_block` rows, block b to rank b % world; local row k
 *   of a rank is global row j = ((k / row_block) * world + rank) * row_block + k % row_block.
 * bands = 1: frame f of the call (0-based) is cut into `world` contiguous bands of `row_block`
 *   rows (the last one shorter; row_block * world >= height) and the rank renders band
 *   (rank + f) mod world: local row k is global row j = band * row_block + k, every frame has
 *   row_block local rows, those with j >= height are not rendered (their RGB8 positions, the
 *   first ones of the frame's buffer, are not written).  Rotating the band from frame to frame
 *   keeps ranks balanced over a batch; a band is a contiguous slice of the frame's PPM body, so
 *   an owner rank can receive it in place (no un-interleave). */
typedef struct {
    uint32_t row_block, rank, world;
    uint32_t bands;
} ceres_tiling;

/* ---- host-side scene preparation (what static.cpp / anim.cpp run before render()) ---- */

/* obj::load_from_file<float> (obj_norms.hpp:120-127 / load_from_stream :57-118): v/f lines,
 * fan triangulation, area-weighted left-handed vertex normals.  *tri48 / *norm36 are
 * malloc'd (free with ceres_free).  An unreadable file yields n_tri = 0 like the reference. */
int ceres_obj_load(const char* path, float** tri48, float** norm36, size_t* n_tri);
/* Procedural heightfield mesh of the C5 configuration (n x n vertices, 2(n-1)^2 triangles,
 * SURVEY.md §8(d)); same arrays as ceres_obj_load. */
int ceres_proc_mesh(int n, float** tri48, float** norm36, size_t* n_tri);
/* rotate_triangles<Axis> (render.hpp:24-44); axis 0/1/2 = x/y/z.  In place. */
int ceres_rotate_triangles(float* tri48, size_t n_tri, int axis, float degrees);
/* compute_bounding_boxes_and_centers + BinnedSahBuilder<Bvh,16>::build (utilities.hpp:142-171,
 * binned_sah_builder.hpp:39-234).  *nodes32 (n_nodes x 32 B) / *prim64 malloc'd. */
int ceres_bvh_build(const float* tri48, size_t n_tri, uint32_t** nodes32, size_t* n_nodes, uint64_t** prim64);
/* The same BinnedSahBuilder<Bvh,16> build on the GPU: identical topology,
 * boxes and primitive_indices as ceres_bvh_build (node numbering is breadth-first for the top,
 * then subtree-contiguous, as the reference's own numbering is OpenMP-timing dependent).
 * ceres_bvh_build_gpu: host buffers in/out, same outputs as ceres_bvh_build, on HIP `device`.
 * ceres_bvh_build_device: d_tri48 in device memory; d_nodes32 holds 2*n_tri-1 nodes (8 u32 each),
 * d_prim32 n_tri u32; stream-ordered on `stream` (a hipStream_t), returns once *n_nodes is known. */
int ceres_bvh_build_gpu(const float* tri48, size_t n_tri, uint32_t** nodes32, size_t* n_nodes, uint64_t** prim64,
                        int device);
int ceres_bvh_build_device(const float* d_tri48, size_t n_tri, uint32_t* d_nodes32, uint32_t* d_prim32,
                           size_t* n_nodes, void* stream);
/* obj::load_from_stream on the GPU: the reference loader's exact triangles
 * and face-order normal sums (obj_norms.hpp:57-118), numbers via glibc-exact strtof/strtol.
 * ceres_obj_load_gpu: same contract as ceres_obj_load (file read on the host, parsed on HIP
 * `device`, malloc'd outputs).  ceres_obj_parse_device: device text in; *d_tri48 / *d_norm36
 * are device arrays (free with ceres_device_free), NULL when the mesh is empty.  A face
 * referencing a missing vertex (the reference's assert, obj_norms.hpp:90) returns CERES_EIO. */
int ceres_obj_load_gpu(const char* path, float** tri48, float** norm36, size_t* n_tri, int device);
int ceres_obj_parse_device(const char* d_text, size_t len, float** d_tri48, float** d_norm36, size_t* n_tri,
                           void* stream);
/* rotate_triangles<Axis> on device triangles (cos/sin of the angle taken on the host). */
int ceres_rotate_triangles_device(float* d_tri48, size_t n_tri, int axis, float degrees, void* stream);
void ceres_device_free(void* d_ptr);
/* The GPU scene preparation above in a chosen arithmetic (CERES_ARITH_EXACT = the calls above,
 * CERES_ARITH_FMA = the reference's CMake build: contracted triangle normals, vertex-normal
 * normalisation, rotation and SAH costs; bit-identical to the *_arith host calls below). */
int ceres_bvh_build_gpu_arith(const float* tri48, size_t n_tri, uint32_t** nodes32, size_t* n_nodes, uint64_t** prim64,
                              int device, int arith);
int ceres_bvh_build_device_arith(const float* d_tri48, size_t n_tri, uint32_t* d_nodes32, uint32_t* d_prim32,
                                 size_t* n_nodes, void* stream, int arith);
int ceres_obj_load_gpu_arith(const char* path, float** tri48, float** norm36, size_t* n_tri, int device, int arith);
int ceres_obj_parse_device_arith(const char* d_text, size_t len, float** d_tri48, float** d_norm36, size_t* n_tri,
                                 void* stream, int arith);
int ceres_rotate_triangles_device_arith(float* d_tri48, size_t n_tri, int axis, float degrees, void* stream, int arith);
/* Camera basis of render.hpp:91-97: out = {dir[3], image_u*w[3], image_v*w*ratio[3]}. */
int ceres_camera_basis(const float eye[3], const float dir[3], const float up[3], float fov_deg,
                       size_t width, size_t height, float out9[9]);
/* The camera/sun orbit of anim.cpp:76-88 (Transform::rotate, transform.hpp:67-112): per frame,
 * eye, dir and sun are rotated by step_deg about `axis` (up is not); rotate_first = 1 rotates
 * before frame 0 like anim.cpp, 0 starts at the given pose.  Writes n_frames x basis12
 * ({eye, dir, image_u, image_v}, as ceres_camera_basis), n_frames x sun3 and, when dir3 is
 * not NULL, n_frames x the rotated (un-normalised) camera dir. */
int ceres_orbit_cameras(const float eye[3], const float dir[3], const float up[3], const float sun[3],
                        float fov_deg, size_t width, size_t height, const float axis[3], float step_deg,
                        uint32_t n_frames, int rotate_first, float* basis12, float* sun3, float* dir3);
void ceres_free(void* p);
/* The six steps above in a chosen arithmetic, arith = CERES_ARITH_EXACT (= the calls above) or
 * CERES_ARITH_FMA (the reference's own CMake build: obj_norms.hpp's normals, the Triangle
 * constructor's cross product, rotate_triangles, the SAH costs of binned_sah_builder.hpp:98-109,179,
 * the camera basis and Transform contract as GCC contracts them; oracle/contraction_sites.txt). */
int ceres_obj_load_arith(const char* path, float** tri48, float** norm36, size_t* n_tri, int arith);
int ceres_proc_mesh_arith(int n, float** tri48, float** norm36, size_t* n_tri, int arith);
int ceres_rotate_triangles_arith(float* tri48, size_t n_tri, int axis, float degrees, int arith);
int ceres_bvh_build_arith(const float* tri48, size_t n_tri, uint32_t** nodes32, size_t* n_nodes, uint64_t** prim64,
                          int arith);
int ceres_camera_basis_arith(const float eye[3], const float dir[3], const float up[3], float fov_deg,
                             size_t width, size_t height, float out9[9], int arith);
int ceres_orbit_cameras_arith(const float eye[3], const float dir[3], const float up[3], const float sun[3],
                              float fov_deg, size_t width, size_t height, const float axis[3], float step_deg,
                              uint32_t n_frames, int rotate_first, float* basis12, float* sun3, float* dir3, int arith);

/* ---- double precision (render<double>, anim.cpp's -d mode, anim.cpp:146-155) ----
 * The same host steps with Scalar = double: bvh::Triangle<double> (96 B), tri_norms as
 * 3 x Vector3<double> (72 B), bvh::Bvh<double>::Node (6 doubles + 2 x u64 = 64 B); OBJ
 * coordinates are strtof floats widened to double (obj_norms.hpp:78-80). */
int ceres_obj_load_f64(const char* path, double** tri96, double** norm72, size_t* n_tri);
int ceres_proc_mesh_f64(int n, double** tri96, double** norm72, size_t* n_tri);
int ceres_rotate_triangles_f64(double* tri96, size_t n_tri, int axis, double degrees);
int ceres_bvh_build_f64(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes, uint64_t** prim64);
int ceres_camera_basis_f64(const double eye[3], const double dir[3], const double up[3], double fov_deg,
                           size_t width, size_t height, double out9[9]);
int ceres_orbit_cameras_f64(const double eye[3], const double dir[3], const double up[3], const double sun[3],
                            double fov_deg, size_t width, size_t height, const double axis[3], double step_deg,
                            uint32_t n_frames, int rotate_first, double* basis12, double* sun3, double* dir3);
/* The same double steps in a chosen arithmetic (CERES_ARITH_FMA: anim.cpp -d as the reference's
 * CMake build compiles it, -O3 -mavx2 -mfma; pair with CERES_MODE_FMA renders). */
int ceres_obj_load_f64_arith(const char* path, double** tri96, double** norm72, size_t* n_tri, int arith);
int ceres_proc_mesh_f64_arith(int n, double** tri96, double** norm72, size_t* n_tri, int arith);
int ceres_rotate_triangles_f64_arith(double* tri96, size_t n_tri, int axis, double degrees, int arith);
int ceres_bvh_build_f64_arith(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes,
                              uint64_t** prim64, int arith);
int ceres_camera_basis_f64_arith(const double eye[3], const double dir[3], const double up[3], double fov_deg,
                                 size_t width, size_t height, double out9[9], int arith);
int ceres_orbit_cameras_f64_arith(const double eye[3], const double dir[3], const double up[3], const double sun[3],
                                  double fov_deg, size_t width, size_t height, const double axis[3], double step_deg,
                                  uint32_t n_frames, int rotate_first, double* basis12, double* sun3, double* dir3,
                                  int arith);
/* BinnedSahBuilder<Bvh<double>,16> on the GPU (bvh_build64.hip): identical topology, boxes (down to the
 * sign of a zero) and primitive_indices as ceres_bvh_build_f64_arith in the same arithmetic; node
 * numbering is breadth-first for the top, then subtree-contiguous, and deterministic.  No value
 * passes through a float.  The calls mirror the float ones:
 * ceres_bvh_build_f64_gpu(_arith): host buffers in/out, same outputs as ceres_bvh_build_f64, on HIP `device`.
 * ceres_bvh_build_f64_device(_arith): d_tri96 in device memory; d_nodes64 holds 2*n_tri-1 nodes (64 B
 * each), d_prim32 n_tri u32; all three 16-byte aligned; stream-ordered on `stream` (a hipStream_t),
 * returns once *n_nodes is known.  Null / empty / bad arith / misaligned: CERES_EINVAL, 2^31 triangles
 * or more: CERES_EUNSUPPORTED -- refused before anything is launched or written. */
int ceres_bvh_build_f64_gpu(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes, uint64_t** prim64,
                            int device);
int ceres_bvh_build_f64_gpu_arith(const double* tri96, size_t n_tri, uint64_t** nodes64, size_t* n_nodes,
                                  uint64_t** prim64, int device, int arith);
int ceres_bvh_build_f64_device(const double* d_tri96, size_t n_tri, uint64_t* d_nodes64, uint32_t* d_prim32,
                               size_t* n_nodes, void* stream);
int ceres_bvh_build_f64_device_arith(const double* d_tri96, size_t n_tri, uint64_t* d_nodes64, uint32_t* d_prim32,
                                     size_t* n_nodes, void* stream, int arith);

/* ---- device scene ---- */

#define CERES_SCENE_STATS 1u   /* flag: build the kernels' traversal-statistics variant */
#define CERES_SCENE_FIRST_ORDER 2u  /* flag: order the shadow BVH4's inner children for walks that take the
                                     * first passing child, and walk single frames in that order (automatic
                                     * for scenes whose nearest-first stack would cost waves, e.g. C5) */

/* Upload a scene to HIP device `device` (re-laid for the GPU: sibling-pair 64-B node records,
 * triangles permuted into leaf order).  The caller keeps ownership of its host arrays; they
 * may be freed after the call.  Returns NULL on failure (see ceres_last_error).
 * Replaces the (bvh, triangles, tri_norms) arguments of render() (render.hpp:87-88).
 * Limits (CERES_EUNSUPPORTED): below 2^32 triangles and nodes; the shadow-ray BVH4 packs each
 * child in one word, so triangle slots / BVH4 records stay below 2^27.  Leaves of any size are
 * accepted: BinnedSahBuilder leaves hold up to 16 triangles, but a node whose centroids cannot be
 * split (coincident triangles, the depth cap) stays one bigger leaf; the shadow BVH4 stores a
 * leaf of more than 31 triangles as a node of equal-box pieces. */
ceres_scene* ceres_scene_create(const float* tri48, size_t n_tri, const float* norm36,
                                const void* nodes32, size_t n_nodes, const uint64_t* prim64,
                                int device, uint32_t flags);
/* The same scene from arrays already in HBM of `device`: d_tri48 / d_norm36 as
 * above, the BVH as n_nodes x 32-B nodes with u32 primitive_indices (ceres_bvh_build_device's
 * output).  The GPU layout is built on the GPU (records numbered differently from
 * ceres_scene_create; the traversal and every image are identical).  Ordered on `stream`
 * (a hipStream_t; NULL = the scene's own); the caller keeps its buffers. */
ceres_scene* ceres_scene_create_device(const float* d_tri48, size_t n_tri, const float* d_norm36,
                                       const uint32_t* d_nodes32, size_t n_nodes, const uint32_t* d_prim32,
                                       int device, uint32_t flags, void* stream);
/* Double-precision scene (render<double>, anim.cpp -d): tri96 / norm72 / nodes64 / prim64 as
 * produced by the _f64 host calls (or the reference's own Bvh<double>).  Render it with
 * ceres_render_f64 / ceres_render_records_f64; the float render calls reject it. */
ceres_scene* ceres_scene_create_f64(const double* tri96, size_t n_tri, const double* norm72, const void* nodes64,
                                    size_t n_nodes, const uint64_t* prim64, int device, uint32_t flags);
/* The same double scene from arrays already in HBM of `device`: d_tri96 / d_norm72 as above, the BVH as
 * n_nodes x 64-B nodes with u32 primitive_indices (ceres_bvh_build_f64_device's output); d_tri96 and
 * d_nodes64 16-byte aligned.  The tree is validated breadth-first on the GPU (child index out of range,
 * leaf range outside primitive_indices, node reached twice, bad primitive index: NULL and a message),
 * then laid out there (scene_device64.hip): sibling pairs numbered by the rank of their inner node in
 * node order -- differently from ceres_scene_create_f64; every render, record, query, shade, refit
 * and SAH cost is identical.  No BVH4 and no cut table (double scenes have neither).  Ordered on
 * `stream` (NULL = the scene's own); the caller keeps its buffers. */
ceres_scene* ceres_scene_create_f64_device(const double* d_tri96, size_t n_tri, const double* d_norm72,
                                           const uint64_t* d_nodes64, size_t n_nodes, const uint32_t* d_prim32,
                                           int device, uint32_t flags, void* stream);
void ceres_scene_destroy(ceres_scene* scene);
/* depth of the BVH (levels below the root) and the traversal-stack entries the kernels use */
int ceres_scene_info(const ceres_scene* scene, uint32_t* depth, uint32_t* stack_entries,
                     size_t* n_pairs, size_t* device_bytes);
/* shadow-BVH4 traversal-stack bounds: nearest-first walks (any child order) and walks that take
 * the first passing child (after the host's inner-child ordering; device-built scenes: equal) */
int ceres_scene_shadow_stacks(const ceres_scene* scene, uint32_t* nearest_first, uint32_t* first_passing);
/* bytes per LDS traversal-stack entry of a float scene's render / trace / shade kernels: 2 below
 * 2^16 sibling pairs and BVH4 records, 3 below 2^24, else 4 (or a negative ceres_status).  Test hook:
 * CERES_DEBUG_STACK_WIDTH=3|4 in the environment when a scene is created makes that scene at least
 * that wide, for good (a rebuild keeps it); the answers do not depend on the width. */
int ceres_scene_stack_width(const ceres_scene* scene);

/* ---- refit: the same scene after its triangles have moved (since 0.4) ----
 * bvh::HierarchyRefitter (hierarchy_refitter.hpp:17-32, with the usual leaf update) on the scene's own
 * layout, in place of destroying and recreating the scene.  New triangle records (and optionally
 * normals) in ORIGINAL triangle order, same n_tri as at creation.  Topology, leaf assignment and record
 * numbering are kept; every box is recomputed, in the scene's scalar type:
 *   a leaf's box   the union over its triangles of Triangle::bounding_box() (triangle.hpp:36-44: the
 *                  points p0, p0 - e1, p0 + e2);
 *   an inner box   the union of its two children's boxes (bounding_box.hpp:23-26);
 *   the root box   the union of the root's two children (what the early-miss test and the background
 *                  cull use); float scenes: every shadow-BVH4 child box = the box of the BVH2 node it
 *                  stands for, and a compressed CERES_MODE_QBVH4 copy is dropped and requantised by the
 *                  next such render.
 * Only min / max is involved: the boxes are exact and independent of evaluation order (a bound that is
 * zero may carry either sign).  The BVH4 keeps its creation-time topology, which stays exact: after a
 * refit every child lies inside its parent.  Every query afterwards (render, records, trace, shade)
 * answers as a scene created from the moved triangles over the refitted BVH would.  What a refit does
 * not repair is tree QUALITY: the topology was built for the old positions, so traversal cost grows with
 * the deformation -- ceres_scene_sah_cost measures it, ceres_scene_rebuild* rebuilds the tree behind the
 * same handle and ceres_scene_update* refits and rebuilds only when it has grown too far ("scene upkeep"
 * below).
 * norm == NULL keeps the scene's normals.  n_tri != the scene's, a null scene or triangle pointer, a
 * float call on a double scene or the reverse: CERES_EINVAL, scene untouched.  Finite coordinates are
 * the contract; non-finite ones give meaningless boxes but no index depends on a coordinate.
 * The *_device calls take DEVICE pointers on the scene's device (triangles 16-byte aligned, otherwise
 * CERES_EINVAL) and enqueue on `stream` (a hipStream_t; NULL = the default stream), where they follow the
 * work already enqueued there.  They SYNCHRONISE that stream once at the end: a float scene's new root
 * box (24 bytes) is read back because later launches receive it by value, so every launch made after
 * the call returns, on any stream, sees the refitted scene.  Renders and queries of the scene still in
 * flight on OTHER streams when the call is made are the caller's to order before it.  The first refit
 * of a scene also sorts its records by tree level (one launch and one synchronise per level) and
 * allocates what later refits reuse; the host-array calls stage through a device buffer the scene keeps.
 * The CPU-scene calls do the same to a ceres_cpu_scene (sibling pairs and leaf-order triangles). */
int ceres_scene_refit(ceres_scene* scene, const float* tri48, size_t n_tri, const float* norm36);
int ceres_scene_refit_device(ceres_scene* scene, const float* d_tri48, size_t n_tri, const float* d_norm36, void* stream);
int ceres_scene_refit_f64(ceres_scene* scene, const double* tri96, size_t n_tri, const double* norm72);
int ceres_scene_refit_f64_device(ceres_scene* scene, const double* d_tri96, size_t n_tri, const double* d_norm72,
                                 void* stream);
/* Diagnostic readback of the current boxes (tests, debugging); synchronises the device.  pair k -> 12
 * scalars lb[6], rb[6] (floats, or doubles for a double scene; bvh.hpp:25-30 order); BVH4 record k -> 24
 * floats in Node4 row order: lo_x[4], hi_x[4], lo_y[4], hi_y[4], lo_z[4], hi_z[4], an empty slot
 * holding lo = +inf, hi = -inf.  Either pointer may be NULL; the counts are returned (0 pairs and 0
 * records for a scene whose root is a leaf, 0 records for a double scene). */
int ceres_scene_read_boxes(ceres_scene* scene, void* pair_boxes, size_t* n_pairs, float* node4_boxes, size_t* n_nodes4);

/* ---- scene upkeep: measure the tree, rebuild it in place, refit-or-rebuild (since 0.5) ----
 * A refit keeps a topology built for the old positions; these calls say how far it has degraded and
 * repair it behind the SAME handle -- no new stream, no lost tile orders, workspaces or pinned buffers,
 * and the ceres_scene* other code holds stays valid.
 *
 * ceres_scene_sah_cost: SahBasedAlgorithm::compute_cost (sah_based_algorithm.hpp:21-32, traversal_cost
 * = 1) over the scene's own records, the same for float and double scenes, GPU and CPU:
 *   HA(box) = (d0 + d1) * d2 + d0 * d1 with d = hi - lo (bounding_box.hpp:43-46), in DOUBLE on the stored
 *             bounds (floats widened first);
 *   ROOT    = the union of the root's two child boxes (what a refit makes the root box; a builder's root
 *             box is not always exactly that union, and double scenes keep none, so no stored root box is
 *             read);
 *   cost    = (HA(ROOT) + sum of HA(child box) * w) / HA(ROOT) over both children of every inner node,
 *             w = the triangle count of a leaf child and 1 for an inner child, accumulated in double.
 * A scene whose root is a leaf: cost = its triangle count, no box is read.  The division is done as
 * written: a degenerate root gives inf or NaN with CERES_OK.  Null scene or cost: CERES_EINVAL.  A pure
 * query: nothing a render or query reads is written.  On the GPU it is one pass over the records and a
 * one-workgroup pass over the per-workgroup partials, enqueued on `stream` (NULL = the default stream),
 * which is SYNCHRONISED once; every order of addition is fixed and the grid depends on the record count
 * only, so two calls on an unchanged scene return the same bits (GPU and CPU agree to rounding, not to
 * the bit).  The scene keeps the small partials buffer after the first call.
 *
 * ceres_scene_rebuild*: a new BVH for the moved triangles, in place.  New triangle records in ORIGINAL
 * order, same n_tri as the scene; norm == NULL keeps the scene's normals; arith = CERES_ARITH_EXACT or
 * CERES_ARITH_FMA, the builder's arithmetic.  Float GPU scenes: ceres_bvh_build_device_arith on the
 * moved triangles, the device relayout, and the scene adopts the result exactly as
 * ceres_scene_create_device does -- afterwards it IS the scene that call would make from the moved
 * triangles and their GPU-built BVH with the scene's flags: every render, record, trace and shade, and
 * ceres_scene_info / _shadow_stacks / _read_boxes answer bit for bit as that fresh scene (a scene first
 * made by ceres_scene_create becomes a device-layout scene: records numbered by the device relayout).
 * What was derived from the old topology goes: a compressed CERES_MODE_QBVH4 copy (requantised by the
 * next such render) and the refit's level list (sorted again by the next refit).  What depends on the
 * frame shape or the device only stays: streams, flags, cached tile orders, compaction buffers,
 * workspaces, pinned buffers, counters, timing state, the staging buffer.  Ordering is the refit's: the
 * _device call takes DEVICE pointers on the scene's device (triangles 16-byte aligned), is enqueued on
 * `stream` and synchronises at the end; launches of the scene in flight on OTHER streams are the
 * caller's to order before the call.  The old arrays are released after one device synchronise, never
 * under a launch.  Errors: n_tri != the scene's, a null scene or triangle pointer, misaligned device
 * triangles or a bad arith: CERES_EINVAL; a DOUBLE GPU scene: CERES_EUNSUPPORTED (the in-place
 * rebuild of a double scene is not implemented; recreate it with ceres_scene_create_f64_device); every refusal happens before anything is launched, freed or written, and a
 * failure inside the build or the relayout leaves the scene as it was.  CPU scenes (float and double):
 * ceres_bvh_build_arith / _f64_arith on the moved triangles, then what ceres_cpu_scene_create* does,
 * into the same handle.
 *
 * ceres_scene_update*: the one call per frame of a moving body -- refit (the refit path above,
 * unchanged), measure `cost`, and iff cost > max_ratio * built_cost evaluates true rebuild from the same
 * triangles (a NaN on either side therefore never rebuilds).  built_cost is the scene's baseline: it is
 * unknown at creation (no create call pays for a measurement); when unknown, update measures it on the
 * tree AS IT FINDS IT, before refitting -- so use update from the first movement on, or the baseline is
 * the tree as first seen; a rebuild, through update or ceres_scene_rebuild*, sets it to the new tree's
 * cost.  max_ratio = +inf never rebuilds (a refit plus a measurement); NaN or <= 0: CERES_EINVAL before
 * anything is touched.  When a rebuild follows, the refit's work is wasted; that is accepted, the refit
 * is cheap against the build.  info may be NULL.  Double GPU scenes: CERES_EUNSUPPORTED, as for
 * rebuild; the other errors and the ordering are rebuild's. */
typedef struct {
    double cost;        /* SAH cost after this call's refit, before any rebuild               */
    double built_cost;  /* the baseline it was compared with                                  */
    double new_cost;    /* cost of the scene as the call leaves it (== cost when not rebuilt) */
    int32_t rebuilt;    /* 0 / 1 */
    int32_t reserved;   /* 0 */
} ceres_update_info;
int ceres_scene_sah_cost(ceres_scene* scene, double* cost, void* stream);
int ceres_scene_rebuild_device(ceres_scene* scene, const float* d_tri48, size_t n_tri, const float* d_norm36, int arith,
                               void* stream);
int ceres_scene_rebuild(ceres_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith);
int ceres_scene_update_device(ceres_scene* scene, const float* d_tri48, size_t n_tri, const float* d_norm36, int arith,
                              double max_ratio, ceres_update_info* info, void* stream);
int ceres_scene_update(ceres_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith,
                       double max_ratio, ceres_update_info* info);

/* ---- the hot path ---- */

/* render<float>() (render.hpp:86-156) on host buffers: uploads nothing but the camera,
 * renders on the device, copies back.  pixels (3*W*H floats) and/or rgb8 (3*W*H bytes, PPM
 * body) may be NULL.  basis12 = {eye[3], dir[3], image_u[3], image_v[3]} as produced by
 * ceres_camera_basis (so libm stays on the host and is pinned by fixtures). */
int ceres_render_f32(ceres_scene* scene, const float basis12[12], const float sun[3], int mode,
                     float* pixels, uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats);

/* Device-resident variant for benchmarks and multi-GPU drivers: all output pointers are
 * DEVICE pointers on the scene's device, work is enqueued on `stream` (a hipStream_t, NULL =
 * default stream) and NOT synchronised.  Launches of one scene may be in flight on several
 * streams at once (bench.py does) as long as only one of them at a time passes d_counters.  Outputs cover only this rank's rows (ceres_tiling):
 * d_pixels = 3*W*local_rows floats (local row-major, local row 0 first) or NULL;
 * d_rgb8 = 3*W*local_rows bytes with local row k stored at position local_rows-1-k (so for
 * world = 1 it is exactly the PPM body) or NULL.  d_counters (8 x u64, zeroed by this call)
 * receives {rays, hits, primary_rays, shadow_rays, node_pairs, tri_tests, error word, 0}; may be
 * NULL.  The error word is 0 for a good render (bit 0: traversal stack overflow; bit 1: a batch
 * launch's compacted tile order did not keep the tiles the host sized its grid for). */
int ceres_render_device(ceres_scene* scene, const float basis12[12], const float sun[3], int mode,
                        size_t width, size_t height, const ceres_tiling* tiling,
                        float* d_pixels, uint8_t* d_rgb8, uint64_t* d_counters, void* stream);
/* A batch of `frames` (1..64) frames of one scene in ONE launch pair -- the render() call
 * that anim.cpp:93-110 makes once per orbit frame, batched.  basis12 = frames x 12 floats
 * (eye, dir, iu, iv per frame), sun3 = frames x 3 floats.  Frame f of the batch occupies
 * d_pixels[f*3*W*local_rows ...] / d_rgb8[f*3*W*local_rows ...], each laid out exactly as
 * ceres_render_device's; counters are summed over the batch.  Every frame keeps its own
 * camera and sun, and its pixels are bit-identical to a single-frame render. */
int ceres_render_batch_device(ceres_scene* scene, uint32_t frames, const float* basis12,
                              const float* sun3, int mode, size_t width, size_t height,
                              const ceres_tiling* tiling, float* d_pixels, uint8_t* d_rgb8,
                              uint64_t* d_counters, void* stream);
/* Multi-GPU frame assembly (device pointers, async on `stream`): d_gathered holds `world`
 * rank buffers, rank r at byte offset r * rank_stride_bytes, each = that rank's d_rgb8 output
 * of a ceres_render_batch_device call with tiling {row_block, r, world} (F frames back to
 * back).  Writes F PPM bodies (F x 3*W*H bytes) to d_out.  This is the un-interleave after the
 * RCCL gather to rank 0; the reference renders on one host (render.hpp:104). */
int ceres_assemble_rgb8(const uint8_t* d_gathered, size_t rank_stride_bytes, uint8_t* d_out, uint32_t frames,
                        size_t width, size_t height, uint32_t row_block, uint32_t world, void* stream);
/* number of HIP devices visible to this process (negative CERES_E* on error) */
int ceres_device_count(void);
/* render<float>() of one frame split over `world` GPUs in ONE process (`./render --gpus N`):
 * scenes[r] (distinct scene objects, one per rank, each on its own device -- or several on one
 * device for testing) renders rows {row_block, r, world}; the RGB8 rows move peer-to-peer
 * (xGMI) to scenes[0]'s device and are assembled there.  pixels / rgb8 are HOST buffers as in
 * ceres_render_f32 (either may be NULL, not both); the frame is identical to a one-GPU render.
 * stats->ms = wall time of the whole call (render + gather + copy back). */
int ceres_render_multi_f32(ceres_scene* const* scenes, uint32_t world, uint32_t row_block,
                           const float basis12[12], const float sun[3], int mode, float* pixels,
                           uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats);
/* The same un-interleave for PACKED rank buffers (an all-to-all's receive buffer): rank r's
 * `frames` x n_r rows start right after rank r-1's, n_r = ceres_tiling_local_rows of rank r. */
int ceres_assemble_rgb8_packed(const uint8_t* d_gathered, uint8_t* d_out, uint32_t frames, size_t width,
                               size_t height, uint32_t row_block, uint32_t world, void* stream);
/* Per-pixel hit records of one render (host buffers, W*H entries each, pixel = j*W + i):
 * prim = ORIGINAL triangle index of the primary hit or -1 (render.hpp:120), tuv = {t, u, v}
 * of that hit (triangle.hpp:95-115 convention), shadow = -1 (no shadow ray), 0 (lit) or
 * 1 (occluded).  A G-buffer output for parity checks and downstream users. */
int ceres_render_records(ceres_scene* scene, const float basis12[12], const float sun[3], int mode,
                         size_t width, size_t height, int32_t* prim, float* tuv, int8_t* shadow,
                         ceres_stats* stats);
/* rows a rank owns under a tiling */
size_t ceres_tiling_local_rows(size_t height, const ceres_tiling* tiling);
/* render<double>() (render.hpp:86-156 with Scalar = double): pixels = 3*W*H doubles (bottom row
 * first) and/or the RGB8 PPM body, basis12 / sun in double.  Records: t/u/v as doubles. */
int ceres_render_f64(ceres_scene* scene, const double basis12[12], const double sun[3], int mode,
                     double* pixels, uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats);
int ceres_render_records_f64(ceres_scene* scene, const double basis12[12], const double sun[3], int mode,
                             size_t width, size_t height, int32_t* prim, double* tuv, int8_t* shadow,
                             ceres_stats* stats);

/* ---- ray queries: closest hit and occlusion for caller-supplied rays (float scenes; double scenes: below) ----
 * The library layer under render(): SingleRayTraverser::traverse(ray, intersector)
 * (single_ray_traverser.hpp:68-126) for any bvh::Ray<float> (ray.hpp:10-22), with the closest and
 * the any-hit ClosestPrimitiveIntersector (primitive_intersectors.hpp).
 *   ray32  n_rays x {origin[3], direction[3], tmin, tmax} = bvh::Ray<float>, 32 B.  The direction
 *          need not be normalised; t is in units of the given direction, as in the reference.
 *          Non-finite components are legal: their comparisons fail as in the reference.  A NaN
 *          as tmin or tmax makes every box and triangle test of the reference fail (its
 *          robust_max / robust_min return a NaN second operand): such a ray is a miss after one
 *          traversal step, here too -- hits, occlusion and Statistics.
 *   hit16  n_rays x {int32 prim, float t, u, v}: prim = ORIGINAL triangle index (as
 *          ceres_render_records), t / u / v as triangle.hpp:95-115; a miss is {-1, 0, 0, 0}.
 * hits16 != NULL asks for the closest hit of every ray -- the BVH2 walk in the reference's order,
 * the last accepted hit with tmin <= t <= tmax, ties left; occluded != NULL (one uint8 per ray,
 * 0 / 1) for the any-hit answer inside the same window, which equals "the closest query finds a
 * hit" (on the GPU: over the exact shadow BVH4).  Either may be NULL, not both.
 * mode: 0, CERES_MODE_FMA, CERES_MODE_ROBUST or both (anything else: CERES_EINVAL); a double scene:
 * CERES_EUNSUPPORTED (use the _f64 calls); n_rays = 0: a successful no-op; n_rays >= 2^31: CERES_EUNSUPPORTED.
 *
 * ceres_trace_rays_device: every pointer is a DEVICE pointer on the scene's device (rays and hits
 * 16-byte aligned); the work is enqueued on `stream` and NOT synchronised, like
 * ceres_render_device, and calls of one scene may be in flight on several streams, each with its
 * own d_counters.  d_counters (8 x u64, zeroed by this call, may be NULL) receives {rays, hits,
 * rays, 0, node_pairs, tri_tests, stack-overflow flag, 0} of the closest query (hits = occluded
 * rays when only occlusion is asked for); node_pairs / tri_tests are filled for
 * CERES_SCENE_STATS scenes and are the reference's Statistics (single_ray_traverser.hpp:132-135).
 * ceres_trace_rays: the same call on host buffers (stats->ms: device time, HIP events).
 * ceres_trace_rays_cpu: the CPU path (OpenMP over rays; threads <= 0: the default), chosen by name
 * only, like ceres_render_cpu_f32; stats->node_pairs / tri_tests always filled, stats->ms wall time. */
int ceres_trace_rays_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, int mode, void* d_hits16,
                            uint8_t* d_occluded, uint64_t* d_counters, void* stream);
int ceres_trace_rays(ceres_scene* scene, const void* rays32, size_t n_rays, int mode, void* hits16, uint8_t* occluded,
                     ceres_stats* stats);

/* ---- all-hits ray queries: every hit in a ray's window, in order (float scenes; double scenes: below) ----
 * What SingleRayTraverser::traverse presents to an intersector that never lowers ray.tmax
 * (single_ray_traverser.hpp:43-63: the window shrinks only through ray.tmax = hit->distance()): the
 * BVH2 walk of :68-126 with every box test against the ray's original [tmin, tmax], every triangle
 * of every reached leaf tested by Triangle::intersect against that window, every accepted triangle
 * a hit.  The hit set is the WALK's -- not "all triangles that pass the triangle test": the fast
 * slab test is not conservative, and a leaf whose box the ray misses is not tested.  With a fixed
 * window the set does not depend on the visiting order.  ray32 / hit16, modes, NaN windows and
 * non-finite components are ceres_trace_rays's.  Per ray:
 *   counts  uint32: the size of the hit set (may exceed max_hits);
 *   hits16  max_hits hit16 records, ray-major (ray r's row starts at record r * max_hits): the
 *           min(count, max_hits) smallest hits by the key -- t ascending by float < ; equal t
 *           (-0 == +0) by ORIGINAL triangle index ascending -- then misses {-1, 0, 0, 0}.  t / u / v
 *           are the bits the closest query reports for that ray and triangle.
 * max_hits: 1 .. CERES_MAX_HITS with a hit buffer (0 or above it: CERES_EINVAL); hits16 = NULL makes the
 * call a count-only query (max_hits ignored); counts and hits16 both NULL: CERES_EINVAL.  A double
 * scene: CERES_EUNSUPPORTED (ceres_trace_rays_all_f64* below answer it); n_rays = 0: a successful no-op; n_rays >= 2^31: CERES_EUNSUPPORTED; every
 * refusal happens before any launch.  More than CERES_MAX_HITS hits: continue with tmin past the
 * last listed t (hits that tie with it are then lost or repeated) -- or ask for the complete hit
 * lists below, which have no cap.
 *
 * ceres_trace_rays_all_device: DEVICE pointers on the scene's device, rays and hits 16-byte aligned,
 * counts 4-byte aligned (otherwise CERES_EINVAL); enqueued on `stream`, NOT synchronised; calls of
 * one scene may be in flight on several streams, each with its own d_counters (8 x u64, zeroed by
 * the call, may be NULL): {rays, rays with count >= 1, rays, 0, node_pairs, tri_tests,
 * stack-overflow flag, 0}; node_pairs / tri_tests are filled for CERES_SCENE_STATS scenes and are
 * the Statistics the reference would count for this walk (a root-leaf scene counts tests and no
 * steps; a ray rejected at the root box counts one step).  The kept hits live in LDS behind the
 * traversal stack: a scene whose stack and hit list together exceed a workgroup's LDS is refused
 * with CERES_EINVAL (the message states both sizes) -- ask for fewer hits.
 * ceres_trace_rays_all: the same call on host buffers (stats->hits: rays with count >= 1;
 * stats->ms: device time; a set overflow flag: CERES_ESTACK).
 * ceres_trace_rays_all_cpu (below): the CPU path, the independent second implementation. */
#define CERES_MAX_HITS 32
int ceres_trace_rays_all_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, int mode, uint32_t max_hits,
                                uint32_t* d_counts, void* d_hits16, uint64_t* d_counters, void* stream);
int ceres_trace_rays_all(ceres_scene* scene, const void* rays32, size_t n_rays, int mode, uint32_t max_hits,
                         uint32_t* counts, void* hits16, ceres_stats* stats);

/* ---- complete hit lists: every hit of every ray, no cap (float scenes; double scenes: below) ----
 * The hit sets of the all-hits query above -- the same walk, modes, ray32 / hit16 records, NaN windows
 * and non-finite components -- as a compact CSR pair instead of padded rows:
 *   offsets  uint64[n_rays + 1], the exclusive prefix sums of the per-ray counts; offsets[n_rays] is
 *            the total;
 *   hits16   `total` hit16 records; ray r owns [offsets[r], offsets[r + 1]): its WHOLE set in the key
 *            order above (t ascending by float <, equal t with -0 == +0 by original triangle index);
 *            t / u / v are the closest query's bits.  No miss records, no cap.
 * Device flow, every step enqueued and none synchronised:
 *   1. ceres_trace_rays_all_device(..., d_counts, d_hits16 = NULL, ...)      the count-only query;
 *   2. ceres_hit_offsets_device: d_offsets = exclusive scan of d_counts (64-bit sums); d_scratch is the
 *      caller's, at least ceres_hit_offsets_scratch_bytes(n_rays) bytes, 8-byte aligned (less, or
 *      misaligned: CERES_EINVAL); n_rays = 0 writes d_offsets[0] = 0;
 *   3. the caller reads d_offsets[n_rays] and allocates that many records;
 *   4. ceres_trace_rays_lists_device: walks only the rays whose segment is non-empty and writes each
 *      one's records, never outside [offsets[r], min(offsets[r + 1], capacity)); past `capacity`
 *      nothing is written, and a segment that crosses it is left unsorted.
 * The library keeps no per-scene scratch and allocates nothing in these calls, so calls of one scene
 * may be in flight on several streams, each with its own buffers and d_counters (8 x u64, zeroed by
 * the call, may be NULL): {rays, rays with a non-empty segment, rays, records written, node_pairs,
 * tri_tests, stack-overflow flag, segment-mismatch flag}; node_pairs / tri_tests are filled for
 * CERES_SCENE_STATS scenes and count the walks this call ran.  The mismatch flag is raised when a
 * walked ray finds another number of hits than its segment's length (offsets of another query, or a
 * scene changed between the calls): that ray's segment is then unspecified, everything outside it
 * untouched.  Argument rules as ceres_trace_rays_all_device (16-byte aligned rays and hits, modes, a
 * double scene and n_rays >= 2^31: CERES_EUNSUPPORTED, n_rays = 0: a successful no-op); d_offsets 8-byte
 * aligned; d_hits16 may be NULL only with capacity = 0; every refusal happens before any launch.
 *
 * ceres_trace_rays_lists (and ceres_trace_rays_lists_cpu below, the independent CPU path): the whole
 * flow on host buffers.  offsets (n_rays + 1, may be NULL) and *total (may be NULL) are always filled;
 * if capacity < *total no record is written and the call returns CERES_ENOMEM (the message states
 * both numbers): allocate and call again, or ask first with hits16 = NULL, capacity = 0.  stats->rays:
 * the rays; stats->hits: rays with at least one hit; node_pairs / tri_tests: the count pass's (the
 * reference's Statistics summed; CERES_SCENE_STATS scenes on the GPU); a set overflow flag gives
 * CERES_ESTACK, a set mismatch flag CERES_EHIP (it cannot happen with the library's own offsets). */
size_t ceres_hit_offsets_scratch_bytes(size_t n_rays);
int ceres_hit_offsets_device(ceres_scene* scene, const uint32_t* d_counts, size_t n_rays, uint64_t* d_offsets,
                             void* d_scratch, size_t scratch_bytes, void* stream);
int ceres_trace_rays_lists_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, int mode,
                                  const uint64_t* d_offsets, void* d_hits16, uint64_t capacity, uint64_t* d_counters,
                                  void* stream);
int ceres_trace_rays_lists(ceres_scene* scene, const void* rays32, size_t n_rays, int mode, uint64_t* offsets,
                           void* hits16, uint64_t capacity, uint64_t* total, ceres_stats* stats);

/* ---- ray queries on double-precision scenes (ceres_scene_create_f64 / ceres_cpu_scene_create_f64) ----
 * The same two queries with Scalar = double, for scenes whose distances outrun float's 24 bits; the
 * semantics are the float queries', word for word (window, unnormalised direction, t in its units,
 * a NaN tmin or tmax = the empty window, either output NULL but not both).
 *   ray64  n_rays x {origin[3], direction[3], tmin, tmax} = bvh::Ray<double>, 8 doubles, 64 B.
 *   hit32  n_rays x {int32 prim, uint32 reserved = 0, double t, u, v}, 32 B: prim = ORIGINAL triangle
 *          index (as ceres_render_records_f64); a miss is {-1, 0, 0.0, 0.0, 0.0}: all-zero bits after prim.
 * hits32 != NULL: the closest hit, the BVH2 walk in the reference's order (the last accepted hit with
 * tmin <= t <= tmax, ties left, tmax shrinking from the ray's own); occluded != NULL: the any-hit
 * answer inside the same window over the same double BVH2 (there is no double BVH4), which equals
 * "the closest query finds a hit".
 * mode: 0 or CERES_MODE_FMA; CERES_MODE_ROBUST is float-only as for ceres_render_f64
 * (CERES_EUNSUPPORTED); anything else: CERES_EINVAL.  A float scene: CERES_EUNSUPPORTED (the float
 * calls above answer a double scene the same way); n_rays = 0: a successful no-op; n_rays >= 2^31:
 * CERES_EUNSUPPORTED.
 * ceres_trace_rays_f64_device: DEVICE pointers on the scene's device, rays and hits 16-byte aligned
 * (otherwise CERES_EINVAL); enqueued on `stream`, NOT synchronised; calls of one scene may be in
 * flight on several streams, each with its own d_counters (8 x u64, zeroed by the call, may be NULL):
 * {rays, hits, rays, 0, node_pairs, tri_tests, stack-overflow flag, 0}, node_pairs / tri_tests the
 * reference's Statistics of the closest query, filled for CERES_SCENE_STATS scenes (a scene whose
 * root is a leaf counts tests and no steps).  The kernel keeps its u32 traversal stack in LDS,
 * stack_entries x 64 lanes x 4 B per workgroup; a scene too deep for the device's LDS is refused with
 * CERES_EINVAL before any launch.  ceres_trace_rays_f64: the same on host buffers (stats->ms: device
 * time; a stack overflow: CERES_ESTACK).  ceres_trace_rays_cpu_f64 (below): the CPU path. */
int ceres_trace_rays_f64_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, int mode, void* d_hits32,
                                uint8_t* d_occluded, uint64_t* d_counters, void* stream);
int ceres_trace_rays_f64(ceres_scene* scene, const void* rays64, size_t n_rays, int mode, void* hits32, uint8_t* occluded,
                         ceres_stats* stats);

/* ---- all-hits ray queries and complete hit lists on double-precision scenes ----
 * The two queries above with Scalar = double: ray64 records in, hit32 records out (see "ray queries on
 * double-precision scenes"; a miss row entry is {-1, 0, 0.0, 0.0, 0.0}, all-zero bits after prim).  The
 * hit set is the walk's, as above, with Triangle<double>::intersect and the fast node intersector in
 * double: every box test against the ray's original [tmin, tmax], the entry / exit bound of each axis
 * picked by the ray's octant (node_intersectors.hpp:35-47; an inverted box is a miss), a NaN tmin or
 * tmax = the empty window.  Order: t ascending by double < (-0 == +0), equal t by ORIGINAL triangle
 * index.  mode: 0 or CERES_MODE_FMA (CERES_MODE_ROBUST: CERES_EUNSUPPORTED, anything else CERES_EINVAL).
 * A float scene: CERES_EUNSUPPORTED.  Every other rule -- max_hits, the count-only query, n_rays = 0,
 * n_rays >= 2^31, alignment (rays and hits 16 bytes, counts 4, offsets 8), the d_counters layouts, the
 * capacity protocol with CERES_ENOMEM, the mismatch flag, the order of the refusals and "before any
 * launch" -- is the float call's of the same name.  ceres_hit_offsets_device and
 * ceres_hit_offsets_scratch_bytes serve both precisions: the device flow is the count-only
 * ceres_trace_rays_all_f64_device, the scan, the total, then ceres_trace_rays_lists_f64_device.
 * LDS per 64-ray workgroup: (stack_entries + 1) x 256 B of stack, then 768 B per kept hit (an 8-byte
 * plane of t bits and a 4-byte plane of leaf slots, [entry][lane]); a scene whose stack and list exceed
 * the workgroup's LDS is refused with CERES_EINVAL (both sizes in the message); the list call keeps as
 * many entries as fit.  The float-named calls keep refusing a double scene, and the ./render command
 * line has no double all-hits mode: these queries are reached through C and Python. */
int ceres_trace_rays_all_f64_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, int mode, uint32_t max_hits,
                                    uint32_t* d_counts, void* d_hits32, uint64_t* d_counters, void* stream);
int ceres_trace_rays_all_f64(ceres_scene* scene, const void* rays64, size_t n_rays, int mode, uint32_t max_hits,
                             uint32_t* counts, void* hits32, ceres_stats* stats);
int ceres_trace_rays_lists_f64_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, int mode,
                                      const uint64_t* d_offsets, void* d_hits32, uint64_t capacity, uint64_t* d_counters,
                                      void* stream);
int ceres_trace_rays_lists_f64(ceres_scene* scene, const void* rays64, size_t n_rays, int mode, uint64_t* offsets,
                               void* hits32, uint64_t capacity, uint64_t* total, ceres_stats* stats);

/* ---- shaded ray queries: render()'s pixel for caller-supplied rays (float scenes) ----
 * For each ray32 record (see "ray queries"), the body of the reference's pixel loop from render.hpp:114
 * on, with the caller's bvh::Ray{origin, direction, tmin, tmax} in place of ray(camera.eye, view) and
 * the ray's direction in place of `view`:
 *   primary  the closest hit under the ray's own window, exactly as ceres_trace_rays answers it (a
 *            direction of any length, the empty window for a NaN bound, ties left);
 *   miss     the pixel is 0, 0, 0;
 *   hit      normal = normalize(tri.n), p = the hit point with its -0.00001 offset (render.hpp:127-133),
 *            sun_line = normalize(sun - p); the shadow ray is the reference's Ray(p, sun_line), window
 *            [0, FLT_MAX], answered any-hit (on the GPU over the exact shadow BVH4, as the render kernels
 *            answer it; on the CPU by render_rows' own closest-hit walk: only the boolean matters);
 *   blocked  the pixel is 0; otherwise it is smooth_shading(sun_line, the original triangle's vertex
 *            normals, view = the ray's direction AS GIVEN, u, v) (render.hpp:46-84).
 * The direction is never normalised for shading: the reference passes one vector to Ray and to
 * smooth_shading, so a view's primary rays (ceres_camera_rays) give ceres_render_f32's framebuffer bit
 * for bit.  A meaningful specular term needs unit directions; t stays in units of the given direction.
 * One sun position per call (host memory, as ceres_render_device takes it); a non-finite sun behaves
 * as in render() (NaN pixels where a hit would be lit).  mode: 0, CERES_MODE_FMA (the contracted
 * arithmetic of the walks, the hit point, normalize and the shading), CERES_MODE_ROBUST or both.
 * Outputs, each optional, at least one (none: CERES_EINVAL), all in ray order:
 *   pixels  n_rays x 3 float32, 12 B per ray;
 *   rgb8    n_rays x 3 bytes, the PPM quantiser (static.cpp:141-143) of the same floats -- no row
 *           flip: a ray list has no rows;
 *   hits16  the closest query's hit16 records, byte-identical to ceres_trace_rays;
 *   status  one byte per ray: 0 = miss, 1 = hit and lit, 2 = hit and in shadow.
 * n_rays = 0: a successful no-op; n_rays >= 2^31: CERES_EUNSUPPORTED; a bad mode bit: CERES_EINVAL; a
 * double scene: CERES_EUNSUPPORTED (use the _f64 calls below).
 *
 * ceres_shade_rays_device: DEVICE pointers on the scene's device except `sun`; rays and hits 16-byte
 * aligned, pixels 4-byte aligned (otherwise CERES_EINVAL, nothing launched or written); enqueued on
 * `stream` and NOT synchronised; calls of one scene may be in flight on several streams, each with
 * its own d_counters, and the render calls' cached state is not touched.  d_counters (8 x u64, zeroed
 * by this call, may be NULL): {rays = n_rays + primary hits, hits = primary hits + shadowed hits,
 * primary_rays = n_rays, shadow_rays = primary hits, 0, 0, stack-overflow flag, 0} -- rays / hits are
 * the pair render() returns.  CERES_SCENE_STATS scenes are accepted and run the same kernels:
 * node_pairs / tri_tests are reported as 0 on the GPU.
 * ceres_shade_rays: the same call on host buffers (stats->ms: device time; a stack overflow:
 * CERES_ESTACK).  ceres_shade_rays_cpu (below): the CPU path.
 * ceres_camera_rays (host): the W*H ray32 records of a view's primary rays (render.hpp:105-113), ray
 * j*W + i for pixel (i, j), origin = eye, window [0, FLT_MAX], direction normalised, in
 * CERES_ARITH_EXACT or CERES_ARITH_FMA (pair the latter with CERES_MODE_FMA) -- the reference's ray
 * generator as the starting point of a caller's own camera model. */
int ceres_shade_rays_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, const float sun[3], int mode,
                            float* d_pixels, uint8_t* d_rgb8, void* d_hits16, uint8_t* d_status, uint64_t* d_counters,
                            void* stream);
int ceres_shade_rays(ceres_scene* scene, const void* rays32, size_t n_rays, const float sun[3], int mode, float* pixels,
                     uint8_t* rgb8, void* hits16, uint8_t* status, ceres_stats* stats);
int ceres_camera_rays(const float basis12[12], size_t width, size_t height, int arith, void* rays32);

/* ---- shaded ray queries on double-precision scenes: render<double>()'s pixel per ray ----
 * The calls above for a scene of ceres_scene_create_f64, word for word with Scalar = double as
 * render<double> (anim.cpp -d, ceres_render_f64) computes it: ray64 records in (see "ray queries on
 * double-precision scenes"); the primary query is exactly ceres_trace_rays_f64's closest hit; the hit
 * point, its -0.00001 offset and sun_line in double; the shadow ray Ray(p, sun_line) with the window
 * [0, DBL_MAX], answered any-hit over the same double BVH2 (no double BVH4 exists); a lit pixel is
 * smooth_shading<double> with the ray's direction AS GIVEN as `view` -- float helpers (a correctly
 * rounded double pow narrowed to float), double weights, float accumulators.  A view's primary rays
 * (ceres_camera_rays_f64) give ceres_render_f64's framebuffer bit for bit.
 * Outputs, each optional, at least one (none: CERES_EINVAL), all in ray order:
 *   pixels  n_rays x 3 DOUBLES, 24 B per ray: the float colour widened, as in ceres_render_f64's
 *           framebuffer;
 *   rgb8    n_rays x 3 bytes, the quantiser applied to those doubles, no row flip;
 *   hits32  the closest query's hit32 records, byte-identical to ceres_trace_rays_f64;
 *   status  0 = miss, 1 = hit and lit, 2 = hit and in shadow.
 * mode: 0 or CERES_MODE_FMA; CERES_MODE_ROBUST: CERES_EUNSUPPORTED (float-only, as everywhere in the
 * double path); any other bit: CERES_EINVAL.  A float scene: CERES_EUNSUPPORTED.  n_rays = 0: a
 * successful no-op; n_rays >= 2^31: CERES_EUNSUPPORTED; null rays or sun with n_rays > 0: CERES_EINVAL.
 * ceres_shade_rays_f64_device: DEVICE pointers except `sun`; rays and hits 16-byte aligned, pixels
 * 8-byte aligned (otherwise CERES_EINVAL); a traversal stack too deep for the device's LDS:
 * CERES_EINVAL, as ceres_trace_rays_f64_device; every refusal happens before any launch or write.
 * Enqueued on `stream` and NOT synchronised; calls of one scene may be in flight on several streams,
 * each with its own d_counters (8 x u64, zeroed by this call, may be NULL: the float call's layout),
 * and the render calls' state is not touched.  CERES_SCENE_STATS scenes run the same kernels and
 * report node_pairs / tri_tests as 0 on the GPU.
 * ceres_shade_rays_f64: the same call on host buffers.  ceres_shade_rays_cpu_f64 (below): the CPU path.
 * ceres_camera_rays_f64 (host): the W*H ray64 records of a view's primary rays, ray j*W + i, origin =
 * eye, window [0, DBL_MAX], in CERES_ARITH_EXACT or CERES_ARITH_FMA (the latter reaches the reference
 * CMake build's double frames; pair it with CERES_MODE_FMA). */
int ceres_shade_rays_f64_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, const double sun[3], int mode,
                                double* d_pixels, uint8_t* d_rgb8, void* d_hits32, uint8_t* d_status, uint64_t* d_counters,
                                void* stream);
int ceres_shade_rays_f64(ceres_scene* scene, const void* rays64, size_t n_rays, const double sun[3], int mode, double* pixels,
                         uint8_t* rgb8, void* hits32, uint8_t* status, ceres_stats* stats);
int ceres_camera_rays_f64(const double basis12[12], size_t width, size_t height, int arith, void* rays64);

/* ---- indexed ray queries and the coherent ray order (since 0.7) ----
 * Every device query above traces all n_rays records, wavefront w taking rays 64 w .. 64 w + 63 as
 * they lie in memory.  The indexed calls take an INDEX LIST instead: lane i of the launch takes ray
 * d_index[i] and writes that ray's own output slot.  A subset is a short list (trace in rounds, shade
 * only what hit, fill only the survivors' segments) -- nothing is compacted or scattered back; a
 * coherent order is a permutation, which ceres_ray_order_device computes.
 *
 * Each ceres_*_indexed_device call is the _device call of the same family with `d_index, n_index` after
 * n_rays; the eight share these rules:
 *   launch     ceil(n_index / 64) single-wavefront workgroups; lane i loads r = d_index[i].
 *   invalid    an entry r >= n_rays is skipped -- no load, no store, no count -- by a per-lane test, so
 *              no list can address outside the caller's arrays.
 *   outputs    indexed by r, exactly where the plain call puts ray r's answer: hits[r], occluded[r],
 *              counts[r], the row at r * max_hits, the segment [offsets[r], offsets[r + 1]), the pixel
 *              and the status at r.  Outputs of rays not in the list are not touched -- with one
 *              exception: after the lists call the segments of unlisted rays are unspecified (the
 *              segment sort pass runs over all rays' segments).
 *   duplicates trace, all-hits, shade: a duplicate entry writes the same bytes twice (and is counted
 *              twice).  The lists call: the entries must be distinct.
 *   refusals   every refusal of the plain sibling applies unchanged (alignment, modes, the precision
 *              of the scene, max_hits, capacity); then n_index >= 2^31: CERES_EUNSUPPORTED; d_index NULL
 *              or not 4-byte aligned with n_index > 0: CERES_EINVAL; a scene created with
 *              CERES_SCENE_STATS: CERES_EUNSUPPORTED (statistics are the plain calls' job).  All before
 *              any launch or write.  n_index = 0: a successful no-op.
 *   counters   d_counters[0] and [2] are n_index as given, [1] counts hits among the traced entries,
 *              [6] is the overflow flag (lists: [3] and [7] as the plain call); with a full permutation
 *              every word equals the plain call's.
 * DEVICE pointers; enqueued on `stream` and NOT synchronised, as their plain siblings.
 *
 * The coherent order.  d_order receives a permutation of 0 .. n_rays - 1, sorted by a 32-bit key with
 * equal keys in ray-index order: one fixed array for given inputs, the one ceres_ray_order_cpu writes.
 * The key reads the ray and the scene's order box (the union of the root's two child boxes) only --
 * not `mode` -- and a poor key can change a run time, never an answer:
 *   bit 31      dead: a NaN among the ray's 8 numbers, a non-finite origin or direction, a zero
 *               direction, !(tmin <= tmax), or an empty interval of the plain slab test against the
 *               box over [tmin, tmax] (an axis with d = 0 passes iff lo <= o <= hi); key 0x80000000;
 *   bits 30..28 the octant (sign bits of d.x, d.y, d.z; bit 28 = x);
 *   bits 27..7  the 21-bit Morton code of the cell of o + t0 d (t0: the interval's start, clamped into
 *               the box) on a 128^3 grid over the box; an axis of zero extent gives cell 0;
 *   bits 6..0   0.
 * When the root is a leaf or the box is not finite (soups with NaN triangles), the slab test is
 * skipped, no ray is dead by it and every cell is 0.
 * ceres_ray_order_scratch_bytes: host arithmetic only (no device needed), non-decreasing in n_rays.
 * ceres_ray_order_device / _f64_device: the scratch is the caller's, 16-byte aligned and at least that
 * large (else CERES_EINVAL); rays 16-byte, d_order 4-byte aligned; the float call refuses a double
 * scene and the double call a float scene (CERES_EUNSUPPORTED); n_rays = 0: a successful no-op;
 * enqueued on `stream`, NOT synchronised, nothing allocated, no per-scene state (several streams may
 * order at once, each with its own scratch).
 * ceres_trace_rays_coherent / _f64: ceres_trace_rays / ceres_trace_rays_f64 on host arrays with the
 * order computed and the indexed kernel launched; the answers are byte-identical to the plain call's,
 * stats->ms covers order plus trace.  CERES_SCENE_STATS scenes: CERES_EUNSUPPORTED.  The host forms of
 * all-hits, lists and shade have no coherent variant: the device calls are the interface for them. */
int ceres_trace_rays_indexed_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, const uint32_t* d_index, size_t n_index,
                                    int mode, void* d_hits16, uint8_t* d_occluded, uint64_t* d_counters, void* stream);
int ceres_trace_rays_all_indexed_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, const uint32_t* d_index,
                                        size_t n_index, int mode, uint32_t max_hits, uint32_t* d_counts, void* d_hits16,
                                        uint64_t* d_counters, void* stream);
int ceres_trace_rays_lists_indexed_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, const uint32_t* d_index,
                                          size_t n_index, int mode, const uint64_t* d_offsets, void* d_hits16, uint64_t capacity,
                                          uint64_t* d_counters, void* stream);
int ceres_shade_rays_indexed_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, const uint32_t* d_index, size_t n_index,
                                    const float sun[3], int mode, float* d_pixels, uint8_t* d_rgb8, void* d_hits16,
                                    uint8_t* d_status, uint64_t* d_counters, void* stream);
int ceres_trace_rays_f64_indexed_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                        size_t n_index, int mode, void* d_hits32, uint8_t* d_occluded, uint64_t* d_counters,
                                        void* stream);
int ceres_trace_rays_all_f64_indexed_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                            size_t n_index, int mode, uint32_t max_hits, uint32_t* d_counts, void* d_hits32,
                                            uint64_t* d_counters, void* stream);
int ceres_trace_rays_lists_f64_indexed_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                              size_t n_index, int mode, const uint64_t* d_offsets, void* d_hits32,
                                              uint64_t capacity, uint64_t* d_counters, void* stream);
int ceres_shade_rays_f64_indexed_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, const uint32_t* d_index,
                                        size_t n_index, const double sun[3], int mode, double* d_pixels, uint8_t* d_rgb8,
                                        void* d_hits32, uint8_t* d_status, uint64_t* d_counters, void* stream);
size_t ceres_ray_order_scratch_bytes(size_t n_rays);
int ceres_ray_order_device(ceres_scene* scene, const void* d_rays32, size_t n_rays, uint32_t* d_order, void* d_scratch,
                           size_t scratch_bytes, void* stream);
int ceres_ray_order_f64_device(ceres_scene* scene, const void* d_rays64, size_t n_rays, uint32_t* d_order, void* d_scratch,
                               size_t scratch_bytes, void* stream);
int ceres_trace_rays_coherent(ceres_scene* scene, const void* rays32, size_t n_rays, int mode, void* hits16, uint8_t* occluded,
                              ceres_stats* stats);
int ceres_trace_rays_coherent_f64(ceres_scene* scene, const void* rays64, size_t n_rays, int mode, void* hits32, uint8_t* occluded,
                                  ceres_stats* stats);

/* ---- closest-point queries (since 0.8) ----
 * For each of the caller's POINTS the nearest point of the scene's surface: how far a position is
 * from the body and where, which facet a sample is closest to, a distance field on a grid.  Float
 * scenes; every tree the library builds, refits or rebuilds.
 *
 * Records.  point16 = {x, y, z, r2max}, four floats: r2max is the squared search radius, +inf for
 * none.  near16 = {int32 prim, float d2, float u, float v}: prim the ORIGINAL triangle index, d2 the
 * squared distance, u and v the weights of p1() and p2() of the closest point -- the hit records'
 * convention, point = (1 - u - v) p0 + u p1 + v p2.  Nothing found: {-1, 0, 0, 0}.
 *
 * The answer does not depend on the BVH or on the order it is walked in: it is, bit for bit, the
 * minimum over ALL triangles of one float formula, in the contraction-free arithmetic both toolchains
 * compile (IEEE division, denormals kept), so a brute force over the triangles reproduces it.
 *   per triangle  a = p0, b = p0 - e1, c = p0 + e2, ab = -e1, ac = e2.  Ericson, Real-Time Collision
 *                 Detection 5.1.5, his regions in his order (vertex a, vertex b, edge ab, vertex c,
 *                 edge ac, edge bc, interior) with his <= / >= tests on d1 .. d6, va, vb, vc; every
 *                 dot product is (x x' + y y') + z z'; the weights (v, w):
 *                   vertex a (0, 0); vertex b (1, 0); edge ab (d1 / (d1 - d3), 0); vertex c (0, 1);
 *                   edge ac (0, d2 / (d2 - d6)); edge bc: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),
 *                   v = 1 - w; interior: denom = 1 / ((va + vb) + vc), v = vb denom, w = vc denom.
 *                 q = (a + ab v) + ac w, then clamped componentwise into the triangle's own bounding
 *                 box min / max(a, b, c) (x < lo ? lo : x > hi ? hi : x); d = p - q,
 *                 d2 = (dx dx + dy dy) + dz dz.  The record's u, v are v, w before the clamp.
 *   selection     best = r2max, prim = -1; a triangle replaces the best iff d2 < best ||
 *                 (d2 == best && (prim < 0 || orig < prim)): a surface at exactly r2max counts, equal
 *                 distances go to the smallest original index, a NaN d2 (a degenerate triangle's
 *                 interior branch, a NaN input) is never taken.  A NaN or negative r2max, or a NaN
 *                 coordinate, is therefore a miss.
 *   pruning       a box's bound is (ex ex + ey ey) + ez ez with e = p - clamp(p, box); a child is
 *                 skipped iff bound > best, strictly.  q lies in every box that contains its triangle's
 *                 box, so per axis |p - clamp(p, box)| <= |p - q| exactly, and float -, * and + are
 *                 monotone: the computed bound is <= the computed d2 of every triangle below the box,
 *                 and nothing that could win or tie is skipped.
 * For a caller-supplied BVH whose boxes do not contain their triangles' boxes the answer is
 * unspecified, as a ray's is.  Finite coordinates are the contract; non-finite triangles give
 * meaningless answers and nothing worse: every index is range-checked, prim stays in [-1, n_tri).
 *
 * ceres_closest_points_device: DEVICE pointers, 16-byte aligned; enqueued on `stream` and NOT
 * synchronised.  d_counters (8 x u64, zeroed by the call, may be NULL): {points, found, points, 0,
 * node_pairs, tri_tests, stack overflow flag, 0}; [4] and [5] are filled on CERES_SCENE_STATS scenes
 * only and their values are implementation-defined (nothing pins the visiting order).
 * ceres_closest_points_indexed_device: lane i takes point d_index[i] and writes near16[d_index[i]], under
 * the rules of "indexed ray queries" above (entries >= n_points skipped, CERES_SCENE_STATS scenes refused,
 * counters[0] and [2] are n_index).
 * ceres_closest_points: HOST arrays, synchronous; stats->rays = points, hits = found, node_pairs /
 * tri_tests where counted, ms the device time; a stack overflow is CERES_ESTACK.
 * Refusals, before anything is launched or written: a null scene or output, null points with
 * n_points > 0, device pointers not 16-byte aligned, a scene whose stack does not fit a workgroup's LDS:
 * CERES_EINVAL; n_points >= 2^31, a double scene: CERES_EUNSUPPORTED.  n_points = 0 is CERES_OK and
 * touches nothing. */
int ceres_closest_points_device(ceres_scene* scene, const void* d_points16, size_t n_points, void* d_near16,
                                uint64_t* d_counters, void* stream);
int ceres_closest_points_indexed_device(ceres_scene* scene, const void* d_points16, size_t n_points, const uint32_t* d_index,
                                        size_t n_index, void* d_near16, uint64_t* d_counters, void* stream);
int ceres_closest_points(ceres_scene* scene, const void* points16, size_t n_points, void* near16, ceres_stats* stats);

/* ---- closest-point queries on double-precision scenes ----
 * The same query on a double scene (ceres_scene_create_f64 and its siblings), where float runs out: a
 * point 10^7 units from metre-sized facets has a float ulp of 1.
 *
 * Records.  point32 = {x, y, z, r2max}, four doubles (32 B).  near32 = {int32 prim, int32 0, double d2,
 * double u, double v} (32 B, the hit32 shape).  Nothing found: {-1, 0, 0.0, 0.0, 0.0}.
 *
 * Contract.  The formula, region order, clamp into the triangle's own box, selection rule, NaN rules and
 * pruning rule are exactly those of "closest-point queries" above with float replaced by double and the
 * float literals by double literals: every dot product (x x' + y y') + z z', no contraction, IEEE
 * division, denormals kept.  The triangles are the scene's Tri96 records (p1() = p0 - e1, p2() = p0 + e2,
 * in double), the boxes its SiblingPair64 bounds.  A child is skipped iff its bound > best, strictly;
 * equal distances go to the smallest original index; a surface at exactly r2max counts.  The argument
 * that the answer is the minimum over ALL triangles, whatever the tree, uses only the monotonicity of
 * IEEE - * + and the strict prune, and holds in double word for word: a brute force over the triangles
 * in double reproduces the answer bit for bit.
 *
 * The calls, their counters ({points, found, points, 0, node_pairs, tri_tests, stack overflow flag, 0};
 * [4] and [5] on CERES_SCENE_STATS scenes only), the indexed call's rules and the order of the refusals
 * are those of the float calls; a float scene is CERES_EUNSUPPORTED ("the _f64 closest-point calls take
 * double scenes").  The walk's LDS stack takes 4 B per entry per lane (a pair index; the float kernel's plane
 * of bounds is compiled out): 256 B per tree level, 16 KiB for a 64-level tree; a need above
 * the device's LDS per workgroup is CERES_EINVAL with both sizes. */
int ceres_closest_points_f64_device(ceres_scene* scene, const void* d_points32, size_t n_points, void* d_near32,
                                    uint64_t* d_counters, void* stream);
int ceres_closest_points_f64_indexed_device(ceres_scene* scene, const void* d_points32, size_t n_points, const uint32_t* d_index,
                                            size_t n_index, void* d_near32, uint64_t* d_counters, void* stream);
int ceres_closest_points_f64(ceres_scene* scene, const void* points32, size_t n_points, void* near32, ceres_stats* stats);

/* Per-launch device timing: while enabled, every render records HIP events around its one
 * kernel (ceres_fused, or ceres_primary in primary-only mode) on the stream it was launched on.
 * ceres_scene_read_timing synchronises, returns the summed kernel durations (ms; shadow_ms is
 * always 0: primary and shadow rays run in the same kernel) and the number of renders since the
 * last read, and resets. */
int ceres_scene_set_timing(ceres_scene* scene, int enable);
int ceres_scene_read_timing(ceres_scene* scene, double* kernel_ms, double* shadow_ms, uint64_t* renders);

/* Diagnostic: per-wavefront records of the last full-mode render of a CERES_SCENE_STATS scene
 * (one 8x8 tile per wavefront), 8 x u64 each: {start, after the primary rays, end
 * (s_memrealtime, 100 MHz), longest primary chain (node pairs), shadow-loop trips, primary hits,
 * the wavefront's primary node pairs, its shadow node pairs}.  Synchronises the device. */
int ceres_scene_wave_log(ceres_scene* scene, uint64_t* out, size_t max_waves, size_t* n_waves);

/* Diagnostic: the tile order the scene's latest batch launch (2..56 frames) read.  A batch launch
 * of whole frames that culls background tiles drops, on the device and ahead of its kernel, every
 * wavefront group (tiles_per_wave consecutive order entries) whose tiles are all culled.
 * info[8] = {1 if that launch read such a compacted order (0: the plain grid; nothing else is
 * set), the tiles the host sized the grid for, the tiles the device kept, the wavefront groups the
 * device kept, tiles per wavefront group, the XCD dealing's chunk in groups (0: the kept groups
 * stay in source order), the source order's entries, 0}.  order (optional, `cap` words): the
 * compacted order, padded with zeros to a multiple of 8 entries; source (optional, `cap` words): the
 * order it was gathered from.  Entries are pack_tile words (frame << 26 | tile row << 13 | tile
 * column) or linear tile ids, as the launch used.  Synchronises the launch's stream. */
int ceres_debug_compact_order(ceres_scene* scene, uint32_t info[8], uint32_t* order, uint32_t* source, size_t cap);
/* The host half of the same, without a device: for a batch of `frames` (2..56) whole frames of
 * width x height with tiles_per_wave 2, 4 or 8 and one cull rectangle per frame (rects = frames x
 * {i0, i1, j0, j1}: the pixel columns and rows whose rays may reach the scene), info[4] = {the
 * tiles the host would size the compacted grid for, the source order's entries, the XCD dealing's
 * chunk in groups (0: none), flags}; flags bit 0: the entries are pack_tile words; bit 1: the host
 * counts by walking the order (short orders); bit 2: by its subset-box sums (frame-major orders
 * whose frames hold the same whole groups); neither: the host has no cheap count, launches of this
 * order keep the plain grid, and info[0] is every tile.  source (optional, `cap` words): the order
 * the groups are formed on. */
int ceres_debug_kept_tiles(size_t width, size_t height, uint32_t frames, uint32_t tiles_per_wave, const uint16_t* rects,
                           uint32_t info[4], uint32_t* source, size_t cap);

/* Entry nodes: batch launches that compact start a kept tile's primary walk at the lowest common
 * ancestor of the nodes of a 64-node cut whose pixel rectangle reaches the tile (csrc/entry_cut.hpp
 * states the table and the rectangle).  The host entry points need no device.
 * ceres_entry_cut_words: the 32-bit words of a cut table.  Word 0: cut nodes; 1: entry_ok; 4..: per
 * cut node, where its box lives (pair << 1 | side); 68..: the pair record of its children
 * (0xffffffff: a leaf); 132..: the boxes, 6 floats each; 516..: lca[64][64], the pair record the
 * walk starts at; 4868..: that record's depth (0: the root's children); 8964..: the root box.
 * ceres_entry_cut_build: the table of a pair array (n_pairs 64-byte sibling-pair records).
 * ceres_entry_relayout: the pair array of a reference BVH as ceres_scene_create lays it out (pairs64:
 * room for *n_pairs records, or NULL to ask for the count), the original triangle index of every
 * leaf slot (orig, n_tri words, optional) and whether the root is a leaf.
 * ceres_entry_rects: one frame's 64 rectangles {i0, i1, j0, j1} (basis12 = eye, dir, iu, iv) as a
 * launch writes them -- every one "keep" {0, 65535, 0, 65535} when the table's entry_ok is 0.
 * ceres_entry_tiles: per 8x8 tile of a whole frame (row-major, tile row 0 = local row 0), the record
 * its walk starts at; 0xffffffff: no rectangle reaches it, every pixel is a miss. */
size_t ceres_entry_cut_words(void);
int ceres_entry_cut_build(const void* pairs64, size_t n_pairs, uint32_t root_leaf_count, const float root_box[6], uint32_t* table);
int ceres_entry_relayout(const float* tri48, size_t n_tri, const void* nodes32, size_t n_nodes, const uint64_t* prim64,
                         void* pairs64, size_t* n_pairs, uint32_t* orig, uint32_t* root_leaf_count);
int ceres_entry_rects(const uint32_t* table, const float basis12[12], size_t width, size_t height, uint16_t* rects);
int ceres_entry_tiles(const uint32_t* table, const uint16_t* rects, size_t width, size_t height, uint32_t* entries);
/* Debug read-back.  ceres_debug_entry_record(scene, 1): later batch launches run the kernels that
 * also record, per 8x8 tile of the batch ([frame][tile row][tile column]), the record its walk
 * started at (0xffffffff: no rectangle reached the tile; 0xfefefefe: no wavefront looked the tile
 * up -- a culled tile).  ceres_debug_entry_nodes: the scene's cut table (table, optional,
 * ceres_entry_cut_words() words) and, for the latest batch launch, info[8] = {table words, 1 if it
 * used entry nodes, its frames, recorded words (0 unless recording was on), width, height, kept
 * tiles, 0}; rects (optional, cap >= frames x 64 rectangles of 4 values) and entries (optional,
 * cap >= recorded words).  Synchronises the device. */
int ceres_debug_entry_record(ceres_scene* scene, int enable);
int ceres_debug_entry_nodes(ceres_scene* scene, uint32_t info[8], uint32_t* table, uint16_t* rects, uint32_t* entries, size_t cap);
/* Retired tiles: in a launch that uses entry nodes, a tile that is root-culled or that no cut
 * rectangle reaches is written by the fill workgroups, and a wavefront group of such tiles leaves
 * at once.  ceres_debug_retire, for the latest batch launch: info[8] = {1 if it retired tiles (0:
 * nothing else is set), frames, tile rows per frame, mask words per tile row, mask words, flags,
 * width, height}; mask (optional, cap >= mask words): the live mask, [frame][tile row][word], bit
 * (column & 31) of word (column >> 5) set when the tile is neither root-culled nor unreached; flags
 * (optional, cap >= flags): one byte per group slot of the compacted order (ceres_debug_compact_order),
 * 1 when no tile of the group is live.  Synchronises the launch's stream. */
int ceres_debug_retire(ceres_scene* scene, uint32_t info[8], uint32_t* mask, uint8_t* flags, size_t cap);

/* Diagnostic (round 6): the bytes the kernels' own fetch sites moved on `device` since the last
 * reset -- out[8] = {64-B sibling-pair records by vector loads (per lane), BVH4 records by vector
 * loads (per lane), BVH4 records through the scalar cache (per wavefront), triangles by vector
 * loads (per lane), triangles through the scalar cache (per wavefront), shading fetches (hit
 * triangle, orig index, vertex normals), framebuffer stores, tile-order entries}.  Only the
 * counting build (`make count`: libceres_hip_count.so, compiled with -DCERES_COUNTING=1) tallies;
 * the product library returns CERES_EUNSUPPORTED.  Synchronises the device; reset != 0 zeroes the
 * tally afterwards.  No reference counterpart: it prices the build against the reference's
 * Statistics (single_ray_traverser.hpp:132-135). */
int ceres_fetch_counters(int device, uint64_t out[8], int reset);

/* ---- the CPU path (./render --cpu) ----
 * render<float>() on host cores, chosen explicitly -- no call falls back to it.  The scene is the
 * product's layout built on the host (sibling-pair records, leaf-ordered triangles) from the same
 * arrays ceres_scene_create takes; the render walks it in the reference's order
 * (single_ray_traverser.hpp:68-126, shadow rays traced closest-hit like render.hpp:135-136) with
 * the arithmetic of the gfx950 kernels, so images, rays and hits equal the reference's in both
 * arithmetics (CERES_MODE_FMA or not), with CERES_MODE_ROBUST / CERES_MODE_PRIMARY as on the GPU
 * (CERES_MODE_QBVH4: CERES_EUNSUPPORTED).  pixels (3*W*H floats, render.hpp:107 layout) and/or rgb8
 * (the PPM body) may be NULL; stats->node_pairs / tri_tests are the reference's Statistics
 * (single_ray_traverser.hpp:132-135) over all rays, stats->ms the wall time.  threads <= 0: the
 * OpenMP default.  Replaces render<float>() (render.hpp:86-156) for a caller without a GPU. */
typedef struct ceres_cpu_scene ceres_cpu_scene;
ceres_cpu_scene* ceres_cpu_scene_create(const float* tri48, size_t n_tri, const float* norm36, const void* nodes32,
                                        size_t n_nodes, const uint64_t* prim64);
void ceres_cpu_scene_destroy(ceres_cpu_scene* scene);
int ceres_render_cpu_f32(const ceres_cpu_scene* scene, const float basis12[12], const float sun[3], int mode,
                         float* pixels, uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats, int threads);
/* render<double> (anim.cpp -d) on host cores: the double arrays of ceres_scene_create_f64, the
 * reference's mixed precision (double rays and traversal, float shading helpers; render64.hip);
 * CERES_MODE_ROBUST is float-only (CERES_EUNSUPPORTED). */
ceres_cpu_scene* ceres_cpu_scene_create_f64(const double* tri96, size_t n_tri, const double* norm72, const void* nodes64,
                                            size_t n_nodes, const uint64_t* prim64);
int ceres_render_cpu_f64(const ceres_cpu_scene* scene, const double basis12[12], const double sun[3], int mode,
                         double* pixels, uint8_t* rgb8, size_t width, size_t height, ceres_stats* stats, int threads);
/* refit of a CPU scene (see "refit" above): the same semantics on host cores; float call on a double
 * scene or the reverse, or n_tri != the scene's: CERES_EINVAL, scene untouched.  Not to be called
 * while another thread renders the scene. */
int ceres_cpu_scene_refit(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36);
int ceres_cpu_scene_refit_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72);
/* upkeep of a CPU scene (see "scene upkeep" above), float and double scenes alike: the same cost (a
 * serial sum in record order), the rebuild through the host builders (ceres_bvh_build_arith /
 * ceres_bvh_build_f64_arith, then the relayout of ceres_cpu_scene_create*) and the same update rule.  A
 * float call on a double scene or the reverse, n_tri != the scene's, a null scene or triangle pointer,
 * a bad arith, max_ratio NaN or <= 0: CERES_EINVAL, scene untouched.  Not to be called while another
 * thread renders the scene. */
int ceres_cpu_scene_sah_cost(const ceres_cpu_scene* scene, double* cost);
int ceres_cpu_scene_rebuild(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith);
int ceres_cpu_scene_rebuild_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72, int arith);
int ceres_cpu_scene_update(ceres_cpu_scene* scene, const float* tri48, size_t n_tri, const float* norm36, int arith,
                           double max_ratio, ceres_update_info* info);
int ceres_cpu_scene_update_f64(ceres_cpu_scene* scene, const double* tri96, size_t n_tri, const double* norm72, int arith,
                               double max_ratio, ceres_update_info* info);
/* ray queries on host cores (see "ray queries" above) */
int ceres_trace_rays_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, void* hits16,
                         uint8_t* occluded, ceres_stats* stats, int threads);
/* ... and on a double CPU scene: ray64 in, hit32 out (see "ray queries on double-precision scenes") */
int ceres_trace_rays_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, void* hits32,
                             uint8_t* occluded, ceres_stats* stats, int threads);
/* the coherent ray order on the host (see "indexed ray queries and the coherent ray order" above, since
 * 0.7): the same key function and std::stable_sort -- the array ceres_ray_order_device writes.  The
 * float call refuses a double scene and the reverse (CERES_EUNSUPPORTED); null rays or order with
 * n_rays > 0: CERES_EINVAL.  ceres_cpu_scene_order_box: the box the key uses as {lo.xyz, hi.xyz} and
 * whether it is usable (0: the root is a leaf or the box is not finite -- every cell is 0). */
int ceres_ray_order_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, uint32_t* order);
int ceres_ray_order_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, uint32_t* order);
int ceres_cpu_scene_order_box(const ceres_cpu_scene* scene, double box6[6], int* usable);
/* all-hits ray queries on host cores (see "all-hits ray queries" above; float scenes, _f64: double scenes,
 * ray64 in and hit32 out): OpenMP over
 * rays, the same box and triangle tests as ceres_trace_rays_cpu under a fixed window, a sorted
 * buffer per ray; stats->node_pairs / tri_tests always filled, stats->ms wall time. */
int ceres_trace_rays_all_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, uint32_t max_hits,
                             uint32_t* counts, void* hits16, ceres_stats* stats, int threads);
/* complete hit lists on host cores (see "complete hit lists" above): the same walk into a vector per
 * ray, std::sort by the key, a prefix sum over the rays, then the copy into the caller's buffer. */
int ceres_trace_rays_lists_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, int mode, uint64_t* offsets,
                               void* hits16, uint64_t capacity, uint64_t* total, ceres_stats* stats, int threads);
int ceres_trace_rays_all_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, uint32_t max_hits,
                                 uint32_t* counts, void* hits32, ceres_stats* stats, int threads);
int ceres_trace_rays_lists_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, int mode, uint64_t* offsets,
                                   void* hits32, uint64_t capacity, uint64_t* total, ceres_stats* stats, int threads);

/* shaded ray queries on host cores (see "shaded ray queries" above): OpenMP over rays (threads <= 0:
 * the default), the walks, hit point, shading and quantiser of ceres_render_cpu_f32; stats->node_pairs /
 * tri_tests are the sum of both walks, as ceres_render_cpu_f32 counts them; stats->ms wall time. */
int ceres_shade_rays_cpu(const ceres_cpu_scene* scene, const void* rays32, size_t n_rays, const float sun[3], int mode,
                         float* pixels, uint8_t* rgb8, void* hits16, uint8_t* status, ceres_stats* stats, int threads);
/* ... and on a double CPU scene (see "shaded ray queries on double-precision scenes"): the walks, hit
 * point, shading and quantiser of ceres_render_cpu_f64; node_pairs / tri_tests as it counts them. */
int ceres_shade_rays_cpu_f64(const ceres_cpu_scene* scene, const void* rays64, size_t n_rays, const double sun[3], int mode,
                             double* pixels, uint8_t* rgb8, void* hits32, uint8_t* status, ceres_stats* stats, int threads);

/* closest-point queries on host cores (see "closest-point queries" above, since 0.8): the same formula,
 * selection and pruning rule over the CPU scene's pairs, OpenMP over points (threads <= 0: the default) --
 * byte for byte the GPU's answers.  stats->node_pairs / tri_tests always filled, stats->ms wall time.  A
 * double CPU scene: CERES_EUNSUPPORTED. */
int ceres_closest_points_cpu(const ceres_cpu_scene* scene, const void* points16, size_t n_points, void* near16,
                             ceres_stats* stats, int threads);
/* ... and on a double CPU scene (see "closest-point queries on double-precision scenes"): point32 in,
 * near32 out, byte for byte ceres_closest_points_f64's answers.  A float CPU scene: CERES_EUNSUPPORTED. */
int ceres_closest_points_cpu_f64(const ceres_cpu_scene* scene, const void* points32, size_t n_points, void* near32,
                                 ceres_stats* stats, int threads);

/* 64-bit content hash of a byte range (multithreaded; deterministic for a given byte string) --
 * what the drop-in include/ceres/render.hpp uses to honour render.hpp:86-156's per-call reading
 * of the caller's triangles / tri_norms / BVH while uploading a scene only when they change. */
uint64_t ceres_content_hash(const void* p, size_t bytes);

/* Launch-geometry introspection for the roofline accounting in bench.py (kernel names as
 * they appear in rocprofv3 traces). */
const char* ceres_kernel_names(void);

const char* ceres_last_error(void);
/* "ceres-mi355x <version> (gfx950) src <16 hex>": the last field is the sha256 of the sources the
 * library was built from (Makefile build_info.o), which bench.py checks against its own tree. */
const char* ceres_version(void);

#ifdef __cplusplus
}
#endif

#endif /* CERES_RENDER_H */
