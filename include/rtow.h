/*
 * rtow.h — C-ABI of the MI355X path-tracing hot path.
 *
 * This is the drop-in boundary for ONE path of joaotavora/raytracing-one-weekend:
 * the per-pixel sample loop of `rtweekend::render(const Scene&, const Config&)`
 * (reference src/render.h:35, src/render.cpp:135-191).  The reference has no FFI;
 * a maintainer would replace the body of render() below the Scene/Config boundary
 * with: flatten the Scene into `rtow_scene_t`, call `rtow_render()`, and hand the
 * returned per-pixel sums to the unchanged write_color()/PPM loop
 * (src/render.cpp:11-20,182-186).  INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no C++ / torch types;
 *   - every function returns 0 on success or a negative RTOW_E* code and never
 *     throws or aborts across the boundary; `rtow_last_error()` gives the text
 *     (thread-local);
 *   - the caller owns every host pointer for the duration of the call only;
 *   - the context owns all device memory (scene, workspace); one call in flight
 *     per context;
 *   - all geometry and radiance are IEEE binary64, like the reference
 *     (src/vec3.h:6-8: vec3 = glm::dvec3).
 */
#ifndef RTOW_H
#define RTOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTOW_ABI_VERSION 9

/* error codes */
#define RTOW_OK 0
#define RTOW_EINVAL (-1)   /* bad argument / inconsistent scene            */
#define RTOW_ENODEV (-2)   /* no usable HIP device                         */
#define RTOW_EHIP (-3)     /* a HIP runtime call failed                    */
#define RTOW_ENOSCENE (-4) /* render called before a scene was uploaded    */
#define RTOW_EEMPTY (-5)   /* scene has no primitives (reference: UB,
                              src/render.cpp:81)                           */
#define RTOW_ENOMEM (-6)   /* host allocation failed                       */

/* material kinds — Lambertian / Metal / Dielectric (src/common-model.h:124-151) */
#define RTOW_MAT_LAMBERTIAN 0
#define RTOW_MAT_METAL 1
#define RTOW_MAT_DIELECTRIC 2

/* primitive kinds — Sphere / MovingSphere / Triangle (src/oo-primitives.h:26-88) */
#define RTOW_PRIM_SPHERE 0
#define RTOW_PRIM_MOVING_SPHERE 1
#define RTOW_PRIM_TRIANGLE 2

/* arithmetic modes of the device path */
#define RTOW_F64_STRICT 0 /* binary64, no FMA contraction: bit-identical to the CPU oracle */
#define RTOW_F64_FAST 1   /* binary64, FMA contraction allowed (default for speed)         */
#define RTOW_F32 2        /* binary32 rays, small-primitive tests and shading on binary32
                             records; large primitives and pixel sums stay binary64.
                             NOT the reference's arithmetic: a faster preview mode whose
                             parity with the binary64 builds is by tolerance (<= 1/255 mean
                             absolute difference per channel at >= 100 spp)             */

/* closest-hit strategies */
#define RTOW_KERNEL_AUTO 0
#define RTOW_KERNEL_BRUTE 1 /* every ray tests every primitive (wave-uniform stream)   */
#define RTOW_KERNEL_BVH 2   /* every lane walks a threaded (stackless) BVH in LDS       */
#define RTOW_KERNEL_GRID 3  /* every lane walks a uniform grid (3D-DDA) in LDS; falls back
                               to BVH when the scene does not suit a grid              */
#define RTOW_KERNEL_BVH4 4  /* triangle meshes: every lane walks a 4-wide BVH, nearest child
                               first, with a per-lane stack in LDS; the image (or the top of
                               its tree) is staged in LDS.  Falls back to BVH for scenes with
                               spheres, for the f32 preview build and for meshes beyond the
                               format's limits (2^18 triangles).  Both builders make its image:
                               the host collapses its SAH tree, the device builder its LBVH   */
#define RTOW_KERNEL_REFTREE 5 /* opt-in exactness mode (RTOW_F64_STRICT only): every lane walks the REFERENCE's own
                               tree — median split of the insertion-ordered primitive array, leaves of 1..6 whose
                               boxes include the origin, float-rounded triangle boxes, signed-radius sphere boxes
                               (src/render.cpp:73-110, src/common-model.cpp:127-134,168-207) — left before right with
                               the reference's f64 Aabb::hit (src/common-model.h:71-84, `t_max <= t_min` rejects).
                               The other kernels give the reference's image wherever its tree finds the closest hit;
                               this one also where it does not (flat leaf boxes, coordinates beyond float precision,
                               negative radii, exact ties).  Never chosen by RTOW_KERNEL_AUTO: it is slow */

/* Camera state: exactly the private members of the reference Camera after its
 * constructor ran (src/common-model.h:104-112, src/common-model.cpp:136-154). */
typedef struct rtow_camera_t {
  double origin[3];
  double u[3], v[3], w[3];
  double horizontal[3];
  double vertical[3];
  double lower_left_corner[3];
  double lens_radius;
  double t0, t1;
} rtow_camera_t;

/* One material record (src/common-model.h:124-151). */
typedef struct rtow_material_t {
  double albedo[3]; /* Lambertian, Metal                       */
  double fuzz;      /* Metal, Dielectric (already clamped 0..1) */
  double ir;        /* Dielectric index of refraction           */
  int32_t kind;     /* RTOW_MAT_*                               */
  int32_t pad_;
} rtow_material_t;

/* Flattened scene: one packed record array per primitive class (structure of
 * arrays across classes; each record is a small aligned block of doubles so a
 * wave-uniform read is one scalar load and a cooperative tile load is fully
 * coalesced).  `prim_kind/prim_index` keep the insertion order of the
 * reference's single primitive array (src/render.h:23), which the reference
 * BVH build depends on (src/render.cpp:73-110). */
typedef struct rtow_scene_t {
  rtow_camera_t camera;

  int32_t n_spheres;
  const double *sphere_geom;   /* [n_spheres][4]  cx cy cz r            */
  const int32_t *sphere_mat;   /* [n_spheres]     material index        */

  int32_t n_moving;
  const double *moving_geom;   /* [n_moving][8]   c0xyz c1xyz r pad     */
  const int32_t *moving_mat;   /* [n_moving]                            */

  int32_t n_triangles;
  const double *triangle_geom; /* [n_triangles][9] ax ay az bx .. cz    */
  const int32_t *triangle_mat; /* [n_triangles]                         */

  int32_t n_materials;
  const rtow_material_t *materials;

  int32_t n_prims;             /* = n_spheres + n_moving + n_triangles  */
  const int32_t *prim_kind;    /* [n_prims] RTOW_PRIM_* in insertion order */
  const int32_t *prim_index;   /* [n_prims] index into that class's arrays */
} rtow_scene_t;

/* Render parameters.  image_height is derived by the caller exactly as the
 * reference does: int(image_width / aspect_ratio) (src/render.cpp:137).
 *
 * `nstreams` has the meaning of the reference's `nthreads`
 * (src/render.cpp:169-185): the samples of a pixel are split into nstreams
 * equal runs of samples_per_pixel / nstreams samples, each run is summed in
 * sample order into its own partial image, and the partial images are added in
 * run order.  Effective spp = samples_per_pixel / nstreams * nstreams.
 *
 * Random numbers are counter-based: request r of sample s of pixel p (global
 * row-major index, top row first) is ONE Philox4x32-7 block keyed by `seed` — request 0 the
 * sample's pixel jitter, shutter time and lens point, request 1 + b everything bounce b
 * draws (the lens point and the scatter's point of the unit ball are sampled directly, with
 * the distributions of the reference's rejection loops, src/random-utils.cpp:23-41); the image
 * therefore does not depend on nranks, tile_rows or on which lane traced what. */
typedef struct rtow_config_t {
  int32_t image_width;
  int32_t image_height;
  int32_t samples_per_pixel;
  int32_t nstreams;
  int32_t max_child_rays;
  int32_t precision;  /* RTOW_F64_*      */
  int32_t kernel;     /* RTOW_KERNEL_*   */
  int32_t rank;       /* this process's share of the image: horizontal strips of */
  int32_t nranks;     /* tile_rows rows dealt round-robin; strip t belongs to    */
  int32_t tile_rows;  /* rank t % nranks.  nranks=1 → whole image.               */
  uint64_t seed;
  /* Stream range (progressive accumulation, sample-split decompositions).
   * stream_count == 0: all nstreams streams.  Otherwise only streams [stream_first,
   * stream_first + stream_count) are traced; sample indices and random numbers are those of the
   * full render.  accumulate != 0: the new partial images are added onto the sums already in the
   * output buffer, in stream order — rendering [0,a) and then [a,n) with accumulate set gives
   * bit for bit the sums of one call over [0,n). */
  int32_t stream_first;
  int32_t stream_count;
  int32_t accumulate;
  int32_t pad_;
} rtow_config_t;

typedef struct rtow_stats_t {
  uint64_t samples;      /* (pixel, sample) pairs traced by this call            */
  uint64_t segments;     /* ray segments traced (calls of ray_color in the ref.) */
  uint64_t prim_tests;   /* primitive hit tests                                  */
  uint64_t node_tests;   /* BVH box tests (0 for the brute-force kernel)         */
  double kernel_ms;      /* device time of the trace kernel (HIP events)         */
  double total_ms;       /* device time of the whole call (all kernels)          */
  int32_t local_rows;    /* rows of the image owned by this rank                 */
  int32_t kernel_used;   /* RTOW_KERNEL_* actually run                           */
} rtow_stats_t;

typedef struct rtow_ctx rtow_ctx;

int rtow_abi_version(void);
const char *rtow_last_error(void);

/* Bind a context to one HIP device (one process per GPU; no global state). */
int rtow_ctx_create(int device_id, rtow_ctx **out);
void rtow_ctx_destroy(rtow_ctx *ctx);

/* Copy the scene into HBM (and build the device BVH).  The scene stays
 * resident until the next upload or ctx destroy.
 * Ordering: the copies and build kernels are QUEUED on the null stream and the call returns without waiting for
 * them.  A render on the null stream or on a blocking stream is ordered behind them by the runtime; a render on a
 * hipStreamNonBlocking stream (every torch.cuda.Stream() side stream) is ordered behind them by the library (it
 * makes the stream wait for an event recorded behind the upload).  build_info.upload_ms is therefore the host time
 * of the call, not the completion time of the copies. */
int rtow_scene_upload(rtow_ctx *ctx, const rtow_scene_t *scene);

/* Who builds the BVH image at rtow_scene_upload (replaces the reference's BVHNode constructor,
 * src/render.cpp:73-110, which runs on the host inside render()):
 *   HOST_SAH    binned surface-area-heuristic build on the host (best tree)
 *   DEVICE_LBVH on the GPU (csrc/rtow_build.hip): bounds, Morton keys and a radix sort, then (round 5) a binned
 *               surface-area-heuristic build, top-down and level by level — the host builder's algorithm (16 bins
 *               per axis, the split that minimises area x count over the three axes, a stable partition by one
 *               scan per level) with every node of a level handled at once; refit; for a triangle mesh the
 *               4-wide image of the BVH4 kernel (greedy collapse level by level, breadth-first nodes, planes
 *               rounded outwards, records in leaf order); the uniform grid of the GRID kernel is built on the
 *               GPU too (csrc/rtow_build_grid.hip, byte-identical to the host-built image).  Nothing of the
 *               build runs on the host.  The tree is as good as the host's (suzanne: 9.0 node tests per segment
 *               with either; 96,800 triangles: 20.5) and is built in 5 ms for 96,800 triangles against the
 *               host's 12-16 on 16 threads.  RTOW_DEVICE_TREE=ploc|radix selects the earlier device trees
 *               (parallel locally-ordered clustering, 7 % slower to walk; Karras' radix tree, 12 %).
 *   AUTO        (default of a new context) per call of rtow_render / rtow_render_rgb8, which know their config:
 *               the device builder for a scene of triangles only with 16,384 of them or more, the host builder
 *               otherwise (a small mesh: the device's two dozen launches cost more than the host's 0.4 ms;
 *               sphere scenes: the grid).  rtow_scene_upload, which knows no config, takes the host builder
 *               under AUTO.
 * Images are bit-identical with either builder (the closest hit is tree-independent).
 * Takes effect at the next upload; the environment variable RTOW_BUILDER=host|device|auto sets the
 * default of new contexts.  rtow_build_info_t::builder says which one built the resident image. */
#define RTOW_BUILDER_HOST_SAH 0
#define RTOW_BUILDER_DEVICE_LBVH 1
#define RTOW_BUILDER_AUTO 2
int rtow_ctx_set_builder(rtow_ctx *ctx, int32_t builder);

typedef struct rtow_build_info_t {
  int32_t builder;          /* builder that produced the resident BVH image */
  int32_t bvh_nodes;        /* node records (without the END record) */
  int32_t bvh_image_bytes;
  int32_t grid_image_bytes; /* 0 = scene not suited to the grid */
  double bvh_build_ms;      /* HOST_SAH: host wall time; DEVICE_LBVH: wall time of the launch sequence
                               including its two small read-backs */
  double grid_build_ms;     /* host wall time */
  double upload_ms;         /* whole rtow_scene_upload call */
  int32_t bvh4_nodes;       /* 4-wide BVH image (triangle meshes, either builder): nodes, 0 = none */
  int32_t bvh4_image_bytes;
  /* RTOW_KERNEL_REFTREE (built at the first render that asks for it; 0 before): nodes of the reference's
   * tree and its "Total BVH stupid volume" diagnostic (src/render.cpp:36-50,148) */
  int32_t ref_tree_nodes;
  int32_t bvh4_node_bytes;  /* 128: binary32 planes (image staged in LDS whole); 64: binary16 planes in the mesh's own
                               frame (bigger meshes, nodes read from L2); 0 = no 4-wide image */
  double ref_tree_stupid_volume;
  double ref_tree_build_ms;
} rtow_build_info_t;
/* Facts about the last rtow_scene_upload of this context. */
int rtow_build_info(rtow_ctx *ctx, rtow_build_info_t *out);

/* Number of image rows owned by cfg->rank, and their global row numbers
 * (ascending) — pure host arithmetic, usable without a GPU. */
int rtow_local_rows(const rtow_config_t *cfg);
int rtow_local_row_list(const rtow_config_t *cfg, int32_t *rows_out, int32_t capacity);

/* Trace this rank's rows.  `d_rgb_sums` is a DEVICE pointer to
 * local_rows*image_width*3 doubles (row-major, this rank's rows in ascending
 * global order); it receives the per-pixel radiance SUMS over the effective spp,
 * i.e. the reference's `global_image` (src/render.cpp:144,176-180) before
 * write_color divides by spp.  `hip_stream` is a hipStream_t (NULL = default
 * stream); the call enqueues work on it and returns without synchronising,
 * unless `stats` is non-NULL, in which case it synchronises the stream and
 * fills `stats`.
 * Samples are never dropped silently: the trace kernel's end-of-launch protocol has a structural trip bound (never
 * observed to fire); lanes that reach it count themselves in a device word, and every entry point that waits for the
 * device — this one with `stats`, rtow_render, rtow_render_rgb8, rtow_multi_render* — returns RTOW_EHIP instead of
 * RTOW_OK when the word is non-zero.  The asynchronous form (stats == NULL) reports it at rtow_profile_collect. */
int rtow_render_device(rtow_ctx *ctx, const rtow_config_t *cfg, void *d_rgb_sums,
                       void *hip_stream, rtow_stats_t *stats);

/* The same with write_color run on the device (src/render.cpp:11-20): `d_rgb8` is a DEVICE pointer to
 * local_rows*image_width*3 BYTES, the values the reference prints for this rank's rows.  The f64 sums stay in the
 * context's workspace (write_color is fused into the reduce kernel when the render is one launch).  cfg->accumulate
 * must be 0.  Asynchronous on `hip_stream` like rtow_render_device.  (What every rank of rtow_multi_render_rgb8 runs.) */
int rtow_render_device_rgb8(rtow_ctx *ctx, const rtow_config_t *cfg, void *d_rgb8, void *hip_stream,
                            rtow_stats_t *stats);

/* write_color on the device (reference src/render.cpp:11-20): for each of the n_values
 * doubles of `d_rgb_sums`, byte = int(256 * clamp(sqrt(sum / spp_effective), 0, 0.999)) into
 * `d_rgb8` (device pointer, n_values bytes).  Enqueued on `hip_stream`, no sync.  The bytes
 * equal the numbers the reference prints in its P3 file. */
int rtow_tonemap_device(rtow_ctx *ctx, const void *d_rgb_sums, int64_t n_values, int32_t spp_effective,
                        void *d_rgb8, void *hip_stream);

/* Every rtow_render_device call brackets its trace-kernel launch with a HIP event
 * pair on the launch stream (no host sync).  This collects the device time of
 * all launches since the previous collect (it waits for them) and resets the
 * ring: `*kernel_ms_sum` = total trace-kernel milliseconds, `*launches` = how
 * many launches that covers (the ring keeps the first 256 per collect). */
int rtow_profile_collect(rtow_ctx *ctx, double *kernel_ms_sum, int32_t *launches);

/* Diagnostic only: copies the 48 device counters of the last launch (see
 * csrc/rtow_trace_body.h; [8..12] are wave-cycle sums per region and [17..22] a histogram of
 * wave end times, [29..33] the finer regions, when the RTOW_STAMPS diagnostic kernel ran). */
int rtow_debug_counters(rtow_ctx *ctx, unsigned long long *out48);

/* Diagnostic only: the LEVELS a render of `cfg` is cut into on this context — pairs (first sample index,
 * sample count), one work item per pixel and level.  RTOW_F64_STRICT: one level per stream (spp / nstreams
 * samples, the reference's threads, src/render.cpp:151-166), summed in stream order like the reference.  Fast
 * builds: the same samples in levels of ONE length that does not depend on nstreams — the divisor of the sample
 * range nearest RTOW_SCHED_CHUNK (10; RTOW_SCHED_CHUNK_MESH = 16 when the resident scene is a triangle mesh) — so
 * that Config::nthreads keeps its arithmetic meaning without setting the size of a work item (csrc/rtow_capi.cpp,
 * level_plan).  A sample range with no divisor within a factor of two of that length (101, 127: primes) is cut into
 * levels of exactly that length with the remainder added to the LAST level (101 = 9 x 10 + 11).  Returns the number of levels (writes at most
 * `capacity_pairs` of them).  `ctx` may be NULL: the table of a new context (pure host arithmetic, usable
 * without a GPU). */
int rtow_debug_schedule(rtow_ctx *ctx, const rtow_config_t *cfg, uint32_t *out_pairs, int32_t capacity_pairs);

/* Diagnostic only: which specialisation of the GRID trace kernel the last trace launch of `ctx` took: 0 generic, 1
 * static spheres, 2 static + moving spheres, | 4 the two-axis walk of a grid with one layer of cells in y (both cover
 * scenes).  RTOW_NO_SPEC in the environment of rtow_ctx_create keeps 0, RTOW_NO_FLAT keeps the bit 4 clear.
 * RTOW_ENOSCENE before the first launch. */
int rtow_debug_last_spec(rtow_ctx *ctx, uint32_t *out_spec);

/* Diagnostic only: whether the trace kernel of the last trace launch of `ctx` counted statistics (segments, node and
 * primitive tests): 1, or 0 for the instantiation without them, which a render that passes stats == NULL launches where
 * the kernel has one (the GRID scene-class kernels and the BVH4 trip kernels of the binary64 builds).  RTOW_COUNT_ALWAYS=1
 * in the environment of rtow_ctx_create keeps 1.  RTOW_ENOSCENE before the first launch. */
int rtow_debug_last_counted(rtow_ctx *ctx, uint32_t *out_counted);

/* Diagnostic only: the constants block of the GRID walk the host derived from the resident grid image (48 32-bit words;
 * csrc/rtow_walk_consts.h, GridWalkConsts: what the scene-class trace kernels read instead of the image header and the
 * head of its large-primitive list).  Copies min(capacity_bytes, 192) bytes to `out` and returns the block's size in
 * *out_bytes.  All zero when no grid image is resident.  RTOW_ENOSCENE before the first upload. */
int rtow_debug_walk_consts(rtow_ctx *ctx, void *out, int32_t capacity_bytes, int32_t *out_bytes);

/* Diagnostic only (pure host arithmetic, usable without a GPU): the order in which the work queue of a render of
 * `cfg` of `scene` runs its 64-pixel tiles.  table_out[queue position] = tile (row-major over this rank's tile rows;
 * the queue is consumed from its far end, so position 0 runs LAST), empty_out[tile] = 1 when no ray the camera can
 * generate through the tile's pixels (any jitter, any lens point, any shutter time) can reach a primitive.  The empty
 * tiles hold the positions [0, *n_empty): they are traced last.  RTOW_TILE_ORDER=0 in the environment switches the
 * classification off (no tile is reported empty, the order is that of the rows alone).  Returns the number of tiles
 * (0 when the launch is not tiled) and writes at most `capacity` entries of each array. */
int rtow_debug_tile_order(const rtow_scene_t *scene, const rtow_config_t *cfg, uint32_t *table_out, unsigned char *empty_out,
                          int32_t capacity, int32_t *n_empty, int32_t *tile_w_log2, int32_t *tile_h_log2);

/* Diagnostic only: copies a resident scene image to the host (which: 0 BVH image, 1 grid image,
 * 2 / 3 the same of the RTOW_F32 build, 4 the 4-wide BVH image of a triangle mesh, 5 the 48-byte frame record
 * of the 4-wide walk: double c[3], float is[3] (binary16 planes decode as c + h * is per axis), uint32_t half
 * (1: 64-byte nodes with binary16 planes), uint32_t lds_limit (the resident scene's; every launch sets the bytes it
 * stages on its own copy), 4 bytes of padding).  Size 0 for an image that is not
 * resident (4 and 5 without a 4-wide image).  `out` NULL: size query.  The tests compare host-built and
 * device-built images byte for byte with it and check them against the geometry. */
int rtow_debug_image(rtow_ctx *ctx, int32_t which, void *out, int64_t capacity, int64_t *size_out);

/* ---- closest-hit ray queries ------------------------------------------------------------------------------------
 * "What does this ray hit?" against the scene resident in a context: the world hit of the reference
 * (src/render.cpp:33-34,52-71) for caller rays, with the walks and hit tests the render runs.  The render path is not
 * involved: a query neither enters the rtow_profile_collect ring nor touches the dropped-sample word, and a render after
 * any number of queries is bit-identical to one without them. */
typedef struct rtow_ray_t {   /* 64 B: four 16-byte loads per ray */
  double origin[3];
  double time;                /* shutter time: MovingSphere centre = c0 + time*(c1-c0) (src/oo-primitives.h:64-66) */
  double direction[3];        /* need not be normalised; t is in units of |direction|, like Ray::at */
  double tmax;                /* the closest hit is reported if it lies in [0.001, tmax] (tmin: src/render.cpp:33) */
} rtow_ray_t;

typedef struct rtow_hit_t {   /* 72 B */
  double t;                   /* +inf on a miss */
  double point[3];            /* origin + t*direction (Ray::at); 0 on a miss */
  double normal[3];           /* the reference's Hit::normal: spheres normalize(p - c), flipped to face the ray;
                                 triangles the un-normalised e1 x e2 (src/common-model.cpp:83-90,121); 0 on a miss */
  int32_t prim;               /* position in the uploaded scene's insertion order (prim_kind / prim_index; class-major
                                 order — spheres, moving spheres, triangles — for a scene uploaded without one); -1 miss */
  int32_t kind;               /* RTOW_PRIM_*; -1 miss */
  int32_t material;           /* index into rtow_scene_t::materials; -1 miss */
  int32_t front_face;         /* the reference's front_facing (always 1 for a triangle hit); 0 on a miss */
} rtow_hit_t;

/* Closest hit of n_rays rays against the scene resident in ctx.  d_rays / d_hits are DEVICE pointers (rays 16-byte
 * aligned, hits 8-byte aligned).  Enqueued on hip_stream with the ordering rule of rtow_render_device (a
 * hipStreamNonBlocking stream is made to wait for the last rtow_scene_upload); returns without synchronising unless
 * stats != NULL, in which case it synchronises the stream and fills: segments = n_rays, prim_tests, node_tests,
 * kernel_ms (HIP events around the query kernel), total_ms, kernel_used; samples = local_rows = 0.
 *
 *   precision  RTOW_F64_STRICT: t, point, normal and front_face are bit-identical to the reference's hit tests (the
 *                               oracle's), under every kernel;
 *              RTOW_F64_FAST:   the fast build's walks and tests.  Against the reference's hit tests over the real
 *                               numbers (tests/exact_hits.py): on a ray all of whose decisions (edge tests, the
 *                               det >= 1e-6 cut, the discriminant, t against 0.001 and tmax, front_face, the gap to the
 *                               second-nearest hit) are clear of their rounding band |q| > 34 u S_q (u = 2^-53, S_q the
 *                               sum of q's absolute terms), hit / miss, the primitive (one of an exact tie) and
 *                               front_face are exact, t is within 34 u (S_num + |t| S_den) / |den| of the exact root,
 *                               point and normal follow; on any other ray the answer is one the band allows (a
 *                               primitive whose own tests are within it, or a miss where every hit is).  An exactly
 *                               tangent ray (discriminant 0) misses.  GRID walks the unit direction, so its triangle
 *                               cut is det >= 1e-6 |d| (the same cut for |d| = 1);
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     RTOW_KERNEL_AUTO resolves as a render of the resident scene does; BRUTE, BVH, GRID and BVH4 have the
 *              render's fallbacks and residency rules (after the lean upload of rtow_render a strategy whose structures
 *              were not built gives RTOW_ENOSCENE, as rtow_render_device does); kernel_used says what ran.
 *              RTOW_KERNEL_REFTREE is strict only (RTOW_EINVAL otherwise) and builds the reference's tree on first use.
 *   tmax       post-filter: the closest hit over [0.001, inf) is reported when its t <= tmax, else a miss (exact: the
 *              closest hit lies within tmax exactly when any hit does).  The walks are not seeded with tmax, so a
 *              short tmax prunes nothing.  (rtow_first_hits_device with max_hits == 1 is the closest hit with
 *              tmax-seeded walks: the same record wherever the closest t is not an exact tie, for what lies within tmax.)
 *   time       results are independent of the kernel for time in [0, 1] only: the moving spheres' boxes cover that
 *              interval (the reference's BVH has the same property).
 * Errors: RTOW_EINVAL for a NULL ctx, NULL buffers with n_rays > 0, n_rays < 0 or > 2^31 - 64, misaligned buffers, an
 * unknown precision or kernel; RTOW_ENOSCENE without a resident scene.  n_rays == 0 returns RTOW_OK and launches
 * nothing.  One call in flight per context, as for the renders. */
int rtow_intersect_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays,
                          void *d_hits, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_intersect(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays,
                   rtow_hit_t *hits, rtow_stats_t *stats);

/* ---- any-hit (occlusion) ray queries --------------------------------------------------------------------------------
 * "Is there anything between here and there?" — the shadow / visibility test: for every ray, occluded[i] = 1 if some
 * primitive's hit test accepts a t in [0.001, tmax], else 0.  Exactly when rtow_intersect with the same precision and
 * kernel reports a hit (hits[i].t <= tmax), but the walks are seeded with tmax (box and cell culling prune at it from the
 * first node) and a ray stops at its first accepted hit, so a short or occluded ray pays for what it needs only.
 * d_rays: the rtow_ray_t rays of rtow_intersect_device (DEVICE memory, 16-byte aligned); d_occluded: n_rays bytes of
 * DEVICE memory (no alignment; a torch.bool tensor), each written 0 or 1 — nothing beyond n_rays is written.  Enqueued on
 * hip_stream with the ordering rule of rtow_intersect_device; returns without synchronising unless stats != NULL, which
 * synchronises and fills segments = n_rays, prim_tests and node_tests (the tests the any-hit walks ran: BRUTE counts
 * its primitive tests too), kernel_ms, total_ms, kernel_used; samples = local_rows = 0.
 *
 *   precision  RTOW_F64_STRICT: occluded[i] == (rtow_intersect(...).t <= tmax) for every ray, under every kernel (and
 *                               the same under BRUTE, BVH, GRID and BVH4 for time in [0, 1]);
 *              RTOW_F64_FAST:   the fast build's walks; the exact any-hit answer on every ray whose decisions are clear
 *                               of the band of rtow_intersect_device (t against tmax included), an answer the band
 *                               allows on the others; an exactly tangent ray is not occluded by that sphere; GRID's
 *                               triangle cut is det >= 1e-6 |d|;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     as rtow_intersect_device: the same resolution, fallbacks, residency rules (RTOW_ENOSCENE after a lean
 *              upload) and kernel_used; RTOW_KERNEL_REFTREE is strict only (it runs the reference tree's closest hit and
 *              compares it with tmax).
 *   tmax       +inf: "hits anything"; below 0.001, or NaN: 0 (the ray skips the walk).
 * Errors: those of rtow_intersect_device (the result buffer has no alignment requirement).  n_rays == 0 returns RTOW_OK
 * and launches nothing.  The first call after an upload does no host work (no primitive ids to translate).  One call in
 * flight per context, as for the renders; the render path is not involved. */
int rtow_occluded_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays,
                         void *d_occluded /* uint8_t[n_rays] */, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_occluded(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays,
                  uint8_t *occluded, rtow_stats_t *stats);

/* ---- first-k-hits (ordered multi-hit) ray queries -------------------------------------------------------------------
 * "What are the first k things this ray passes through, in order?" — ordered transparency, thickness and layer counts,
 * picking through glass, shadow rays that skip dielectrics, depth peeling — in one launch, without the epsilon a chain
 * of rtow_intersect calls from each hit point needs, and exact where primitives tie.
 *
 *   hit set    For ray i, H is the set of primitives whose reference hit test (Sphere::hit, MovingSphere, Triangle::hit)
 *              accepts a t in [0.001, ray.tmax], each with that t: ONE entry per primitive.  A sphere contributes the
 *              root the reference picks — the near root if it is >= 0.001, else the far root; the exit of a sphere
 *              entered at t is found by a follow-up ray from that hit.  Triangles are hit only where det >= 1e-6, as
 *              everywhere else in the library.
 *   order      H ascending by (t, insertion index) — the insertion index is rtow_hit_t::prim.  The tie rule is part of
 *              the contract: it makes the answer independent of kernel, builder and scheduling, also when a tie
 *              straddles slot max_hits.
 *   output     counts[i] = min(|H|, max_hits); hits[i][j] for j < counts[i] is the full rtow_hit_t of the j-th entry —
 *              exactly the fields rtow_intersect writes for that primitive and ray; slots j >= counts[i] hold the miss
 *              record (t = +inf, zeros, -1, -1, -1, 0).  All max_hits slots of every ray are written; nothing is
 *              written beyond n_rays * max_hits records or beyond n_rays counts.  d_counts may be NULL.
 *   tmax       below 0.001, or NaN: count 0 without a walk.  The walks are seeded with tmax, and once max_hits entries
 *              are kept they cull at the t of the last one (inclusive: every member of a tie is still visited).
 *   max_hits   1 .. RTOW_MAX_HITS.  max_hits == 1 is the closest hit with tmax-seeded walks (see the tmax note of
 *              rtow_intersect_device), ties resolved to the lowest insertion index.
 *   precision  RTOW_F64_STRICT: bit-identical to the definition above under BRUTE, BVH, GRID and BVH4, with either
 *                               builder, for time in [0, 1];
 *              RTOW_F64_FAST:   the fast build's tests and walks.  On a ray all of whose decisions are clear of the
 *                               rounding band of rtow_intersect_device — t against tmax and the gaps between consecutive
 *                               hits up to the first one left out included — the sequence is the exact one; on any
 *                               other ray it is one the band allows.  An exactly tangent ray misses that sphere; GRID's
 *                               triangle cut is det >= 1e-6 |d|.  Reported t is non-decreasing under every walk, and
 *                               bit-equal t come in insertion order under BRUTE, BVH and BVH4.  GRID orders by the
 *                               distance t |d| (insertion index on equal distances) and converts at output, where two
 *                               distances may round to one t: under GRID the order of entries with bit-equal t is not
 *                               guaranteed (observed on coplanar overlapping triangles);
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     AUTO, fallbacks, residency rules (RTOW_ENOSCENE after a lean upload) and kernel_used as in
 *              rtow_intersect_device.  RTOW_KERNEL_REFTREE: RTOW_EINVAL (the reference's tree misses hits by design and
 *              has no multi-hit meaning; as in rtow_closest_point).
 * d_rays: rtow_ray_t, DEVICE memory, 16-byte aligned; d_hits: n_rays * max_hits rtow_hit_t, 8-byte aligned; d_counts:
 * n_rays int32_t, 4-byte aligned, or NULL.  Enqueued on hip_stream with the ordering rule of rtow_intersect_device (a
 * non-blocking stream waits for the last upload or refit); returns without synchronising unless stats != NULL, which
 * synchronises and fills segments = n_rays, prim_tests and node_tests (BRUTE counts the tests it ran), kernel_ms,
 * total_ms, kernel_used; samples = local_rows = 0.
 * Errors: those of rtow_intersect_device; max_hits outside [1, RTOW_MAX_HITS] is RTOW_EINVAL.  n_rays == 0 returns
 * RTOW_OK and launches nothing.  One call in flight per context; the render path, the profile ring and the
 * dropped-sample word are not involved: a render or an rtow_intersect after any number of these calls is bit-identical
 * to one without them. */
#define RTOW_MAX_HITS 8
int rtow_first_hits_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_rays, int64_t n_rays,
                           int32_t max_hits, void *d_hits /* rtow_hit_t[n_rays][max_hits] */,
                           void *d_counts /* int32_t[n_rays] or NULL */, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_first_hits(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_ray_t *rays, int64_t n_rays,
                    int32_t max_hits, rtow_hit_t *hits, int32_t *counts /* or NULL */, rtow_stats_t *stats);

/* ---- closest-point (distance) queries -------------------------------------------------------------------------------
 * "What is the nearest surface to this point?" — for every query point p, the primitive of the resident scene nearest
 * to p, the distance and the nearest point on it, when that distance is <= max_dist.  The geometry is the records the
 * device holds (not the caller's B and C): sphere c and copysign(r^2, r); moving sphere c0 + time * (c1 - c0) with the
 * record's r^2; triangle {a + s e1 + t e2 : s, t >= 0, s + t <= 1} with e1 = B - A, e2 = C - A rounded.  The radius is
 * R = sqrt(|r^2|) (correctly rounded), so a negative radius (hollow glass) is the same surface; the distance to a sphere is
 * | |p - c| - R |, and p at the centre reports c + (R, 0, 0).  A degenerate triangle answers as its edges do; no result
 * is ever NaN for a finite p.  Formulas: csrc/rtow_point_walks.h (the kernel: csrc/rtow_pointq.h).
 *
 *   precision  RTOW_F64_STRICT: dist and point are bit-identical to those formulas evaluated in IEEE binary64 in their
 *                               written order (tests/point_ref.py mirrors them), under every kernel and with either
 *                               builder; prim is one of the primitives whose distance equals the minimum exactly (tie
 *                               rule), and point is that primitive's;
 *              RTOW_F64_FAST:   the same formulas contracted (FMA) with the fast build's square root and reciprocal.
 *                               Against the exact distance D of the reported primitive (tests/point_ref.py):
 *                               D - 64 u S <= dist <= D + 64 u S + min(64 u S k^2, h) (u = 2^-53; S = |p - a|_1 +
 *                               |e1|_1 + |e2|_1 for a triangle, |p - c|_1 + R (+ |c0|_1 + |time (c1 - c0)|_1 when
 *                               moving) for a sphere; k = |e1| |e2| / |e1 x e2|, h the triangle's smallest height; the
 *                               k term is absent for spheres), and that primitive's D is within the same bands of the
 *                               exact minimum.  The strict build meets the same bound with 32 u;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   point      the reported point q of the reported primitive, with tau = 32 u (strict), 64 u (fast):
 *                on the surface: the exact distance from q to the record's exact surface is <= tau S_q, with S_q = |a|_1 +
 *                  |e1|_1 + |e2|_1 for a triangle (q = (a + e1 s) + e2 t: at most 4 roundings per component on magnitudes
 *                  that sum to S_q; edge parameters are clamped to [0, 1], and the plane candidate's s + t exceeds 1 by a
 *                  few u, in the fast build by twice its reciprocal's 4e-15) and S_q = |c|_1 + R (|c0|_1 +
 *                  |time (c1 - c0)|_1 + R when moving) for a sphere (the unit vector's 3 roundings, the root and the
 *                  reciprocal, scaled by R and added to c);
 *                consistent with dist: | |p - q| - dist | <= tau (S + S_q), S as above (dist comes from the residual
 *                  w - e1 s and q from a + e1 s: they differ by their own roundings only).  At a sphere's centre
 *                  q = c + (R, 0, 0) meets both.
 *   overflow   when the exact squared distance exceeds the binary64 range (|p - q| above about 1e154), dist is +inf with a
 *              primitive reported if max_dist is +inf (+inf <= +inf is accepted; which primitive is not specified, and a
 *              finite max_dist reports a miss); point is then finite but need not meet the point clauses (a sphere
 *              reports its centre).  No field is NaN.
 *   kernel     BRUTE tests every primitive; BVH walks the binary tree; BVH4 the 4-wide tree, nearest child first; GRID
 *              has no point walk and is answered by BVH (kernel_used says BVH); AUTO takes BVH4 if the 4-wide image is
 *              resident, else BVH if the binary image is, else BRUTE (so it never fails on a resident scene).  An explicit
 *              BVH4 on a scene without a 4-wide image falls back to BVH, and an explicit BVH whose image was not built by
 *              the lean upload of rtow_render gives RTOW_ENOSCENE, as in the ray queries.  RTOW_KERNEL_REFTREE: RTOW_EINVAL.
 *   max_dist   inclusive, and the walk's starting search radius (a short radius prunes from the first node); NaN or
 *              negative: a miss without a walk; +inf: unbounded.
 *   time       results are independent of the kernel for time in [0, 1] only (the moving spheres' boxes cover it).
 * A miss reports dist = +inf, point 0, prim = kind = material = -1.  prim is the insertion index, as rtow_hit_t::prim.
 * d_queries / d_hits are DEVICE pointers, both 16-byte aligned; nothing beyond n is written.  Enqueued on hip_stream with
 * the ordering rule of rtow_intersect_device; with stats it synchronises and fills segments = n, prim_tests, node_tests,
 * kernel_ms, total_ms, kernel_used.  Errors: those of rtow_intersect_device.  n == 0 launches nothing.  One call in
 * flight per context; the render path (profile ring, dropped-sample word) is not involved. */
typedef struct rtow_point_query_t { /* 48 B, 16-byte aligned in device memory */
  double point[3];
  double time;      /* moving-sphere centre c0 + time*(c1-c0), as in the ray tests */
  double max_dist;  /* report the nearest primitive only if its distance <= max_dist */
  double pad_;
} rtow_point_query_t;

typedef struct rtow_point_hit_t {   /* 48 B */
  double dist;      /* +inf when nothing is within max_dist */
  double point[3];  /* nearest point on that primitive's surface; 0 on a miss */
  int32_t prim;     /* insertion order, exactly as rtow_hit_t::prim; -1 on a miss */
  int32_t kind;     /* RTOW_PRIM_*; -1 on a miss */
  int32_t material; /* -1 on a miss */
  int32_t pad_;
} rtow_point_hit_t;

int rtow_closest_point_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_queries, int64_t n,
                              void *d_hits, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_closest_point(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_point_query_t *queries, int64_t n,
                       rtow_point_hit_t *hits, rtow_stats_t *stats);

/* ---- k-nearest-primitive (ordered distance) queries ------------------------------------------------------------------
 * "What are the k nearest surfaces to this point, nearest first?" — proximity and contact candidates, blending from the
 * few nearest faces, thickness and clearance (first and second nearest), picking near a crease — in one launch.  Queries
 * are rtow_point_query_t and results rtow_point_hit_t, as for rtow_closest_point.
 *
 *   set        For query i, N is the set of primitives whose distance is <= max_dist, the distance computed by the
 *              formulas of rtow_closest_point in the same written order (csrc/rtow_point_walks.h): ONE entry per primitive.
 *   order      N ascending by (dist, insertion index) — the insertion index is rtow_point_hit_t::prim.  The tie rule is
 *              part of the contract, as in rtow_first_hits: it makes the strict answer independent of kernel, builder
 *              and scheduling, also when a tie straddles slot k.
 *   output     counts[i] = min(|N|, k); hits[i][j] for j < counts[i] is exactly the record rtow_closest_point would write
 *              for that primitive (dist, point, insertion index, kind, material); slots j >= counts[i] hold the miss
 *              record (dist = +inf, point 0, prim = kind = material = -1).  All k slots of every query are written;
 *              nothing is written beyond n * k records or beyond n counts.  d_counts may be NULL.
 *   k          1 .. RTOW_MAX_NEAREST; outside that range: RTOW_EINVAL.  k == 1 is rtow_closest_point's answer with the
 *              tie resolved to the lowest insertion index: the same dist always, and the same record whenever both name
 *              the same primitive.  (rtow_closest_point may name any primitive of an exact tie, with that primitive's
 *              point: two triangles tie exactly along a shared edge, and their points there may differ in the last
 *              bits.  Its record is then a later entry of this query's list, at the same dist.)
 *   max_dist   inclusive, and the walk's starting search radius; NaN or negative: count 0 without a walk; +inf:
 *              unbounded.  Once k entries are kept, the search radius is the distance of entry k - 1, and every member of
 *              a tie at that radius is still visited: a box is pruned only beyond (radius + sigma)^2 with the slack sigma
 *              of the closest-point walks, which is above every rounding of a computed distance.  The radius only shrinks.
 *   precision  RTOW_F64_STRICT: bit-identical to the definition above evaluated with the formulas' mirror
 *                               (tests/point_ref.py, tests/nearest_ref.py) under BRUTE, BVH, BVH4 and AUTO, with GRID
 *                               answered by BVH, with either builder, after a refit, for time in [0, 1];
 *              RTOW_F64_FAST:   every reported (dist, prim) meets rtow_closest_point's distance band and point clauses for
 *                               that primitive; dist is non-decreasing; the primitives are distinct; entries with
 *                               bit-equal dist come in insertion order; and the list is complete up to the bands: for
 *                               every unreported primitive c with exact distance D(c) and upper band up(c),
 *                               D(c) + up(c) >= dist[k - 1] when count == k, and D(c) + up(c) >= max_dist when count < k.
 *                               The fast answer is not promised to be the same under every kernel;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 * Overflow, the kernel rules (AUTO, GRID answered by BVH, the BVH4 fallback, RTOW_ENOSCENE after a lean upload,
 * RTOW_KERNEL_REFTREE: RTOW_EINVAL), the stream ordering, stats (segments = n) and errors are those of
 * rtow_closest_point_device.  d_queries and d_hits (n * k rtow_point_hit_t) are DEVICE pointers, 16-byte aligned;
 * d_counts: n int32_t, 4-byte aligned, or NULL.  n == 0 launches nothing.  One call in flight per context; the render
 * path (profile ring, dropped-sample word) is not involved. */
#define RTOW_MAX_NEAREST 8
int rtow_nearest_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_queries, int64_t n,
                        int32_t k, void *d_hits /* rtow_point_hit_t[n][k] */, void *d_counts /* int32_t[n] or NULL */,
                        void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_nearest(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_point_query_t *queries, int64_t n,
                 int32_t k, rtow_point_hit_t *hits, int32_t *counts /* or NULL */, rtow_stats_t *stats);

/* ---- radiance queries ---------------------------------------------------------------------------------------------------
 * "How much light arrives along this ray?" — the reference's ray_color (src/render.cpp:112-129) for caller rays: light
 * probes, lightmap texels, a camera of the caller's own.  For ray i the result is the sum over j = 0 .. samples_per_ray - 1
 * of ray_color(ray_i, max_child_rays), added in sample order by one lane starting from +0.0: SUMS, like
 * rtow_render_device — the caller divides.  A hit with no child rays left is black (src/render.cpp:115).
 *
 *   rays       rtow_ray_t, as for rtow_intersect.  `time` is the path's shutter time and is handed on to every scattered
 *              ray; `tmax` is not read: paths are unbounded, like the reference's.
 *   Philox     sample j of ray i draws as (pixel, sample) = (ids[i][0], ids[i][1] + sample_first + j), the sums mod 2^32;
 *              without ids (NULL) as (i, sample_first + j).  Bounce b draws request 1 + b; request 0 belongs to the
 *              render's camera and is never drawn.  So a ray a render generated for (pixel, sample), queried with that
 *              identity and the render's seed and max_child_rays, gives that sample's colour; and a caller who wants more
 *              parallelism than one lane per ray repeats the ray with different first sample indices.
 *   precision  RTOW_F64_STRICT: bit-identical to the oracle's ray_color on that ray and identity, under every kernel and
 *                               with either builder: attenuations are folded from the end of the path,
 *                               a1*(a2*(...*sky)), as the strict render does;
 *              RTOW_F64_FAST:   the fast build's walks, the forward product ((a1*a2)*...)*sky, contracted arithmetic;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *              In both builds a ray with k samples equals the in-order sum of k one-sample queries bit for bit, and the
 *              result does not depend on how the rays were scheduled.
 *   kernel     as rtow_intersect_device: the same resolution, fallbacks, residency rules (RTOW_ENOSCENE after a lean
 *              upload) and kernel_used; RTOW_KERNEL_REFTREE is strict only.
 * d_rays (16-byte aligned), d_ids (uint32_t[n_rays][2], 8-byte aligned, or NULL) and d_rgb_sums (double[n_rays][3], 8-byte
 * aligned) are DEVICE pointers; nothing beyond n_rays results is written.  Enqueued on hip_stream with the ordering rule
 * of rtow_intersect_device (a non-blocking stream is made to wait for the last upload or refit); returns without
 * synchronising unless stats != NULL, which synchronises and fills samples = n_rays * samples_per_ray, segments (traced,
 * from a device counter), prim_tests, node_tests, kernel_ms, total_ms, kernel_used; local_rows = 0.
 * Errors: RTOW_EINVAL for a NULL ctx or params, NULL rays or result with n_rays > 0, n_rays < 0 or > 2^31 - 64, rays not
 * 16-byte aligned, ids or result not 8-byte aligned, samples_per_ray < 1, max_child_rays < 0, an unknown precision or
 * kernel; RTOW_ENOSCENE without a resident scene.  n_rays == 0 returns RTOW_OK and launches nothing.  One call in flight
 * per context.  The render path is not involved: the profile ring and the dropped-sample word are untouched, and a render
 * after any number of radiance queries is bit-identical to one without them. */
typedef struct rtow_radiance_params_t {   /* 24 B */
  uint64_t seed;            /* Philox key, as rtow_config_t::seed */
  int32_t samples_per_ray;  /* >= 1: paths traced per ray, summed in sample order */
  int32_t max_child_rays;   /* >= 0: the render's depth */
  uint32_t sample_first;    /* added (mod 2^32) to every ray's first sample index */
  int32_t pad_;
} rtow_radiance_params_t;

int rtow_radiance_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_radiance_params_t *params,
                         const void *d_rays, int64_t n_rays, const void *d_ids /* uint32_t[n_rays][2] or NULL */,
                         void *d_rgb_sums /* double[n_rays][3] */, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_radiance(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_radiance_params_t *params,
                  const rtow_ray_t *rays, int64_t n_rays, const uint32_t *ids, double *rgb_sums, rtow_stats_t *stats);

/* ---- path-step queries: one segment per caller ray ---------------------------------------------------------------------
 * "Where does this ray go next, and what does the surface take from it?" — ONE segment of the reference's ray_color: the
 * closest hit, then Material::scatter (src/common-model.cpp:13-62).  It is the stage rtow_radiance keeps to itself, for
 * callers who drive the bounces: their own lights with rtow_occluded shadow rays, Russian roulette, per-bounce AOVs,
 * path-length statistics, another sky, compaction between bounces.  rtow_camera_rays, then rtow_path_step repeated
 * max_child_rays + 1 times with bounce = 0, 1, ... and folded by the caller, IS rtow_radiance (bit for bit in the strict
 * build): colour = a_0 * (a_1 * (... * a_k)) over the attenuations up to the step that ended the path — the sky's colour
 * on a MISS, 0 on ABSORBED, and 0 by the caller's own rule for a hit at bounce == max_child_rays (src/render.cpp:115: the
 * call knows nothing of a depth).
 *
 *   identity   ray i draws as (pixel, sample) = (ids[i][0], ids[i][1] + sample_first), the sum mod 2^32; without ids
 *              (NULL) as (i, sample_first).  The scatter draws request 1 + bounce of that identity, as rtow_radiance does
 *              for the path's segment `bounce`.  bounce is one number per call.
 *   per ray    status[i] is one of
 *     RTOW_STEP_SKIPPED    tmax is NaN or below 0.001: no walk.  atten = 0, hit = the miss record, next = the DEAD RAY:
 *                          every field 0 and tmax = -1.  A dead ray fed back stays dead, so a caller can loop in place
 *                          (d_next == d_rays) without compaction.
 *     RTOW_STEP_MISS       no hit in [0.001, tmax] (tmax is a post-filter, exactly as in rtow_intersect_device: the walks
 *                          are not seeded with it).  atten = the reference's background for the ray
 *                          (src/render.cpp:122-128): (1-t)*1 + t*(0.5, 0.7, 1.0), t = 0.5*(unit(direction).y + 1);
 *                          hit = the miss record; next = the dead ray.
 *     RTOW_STEP_SCATTERED  hit = the record rtow_intersect_device writes for this ray; atten = the hit material's
 *                          attenuation as uploaded; next.origin = hit.point, next.direction = what scatter returns
 *                          (Lambertian normal + rnd, metal reflect(d, n) + fuzz*rnd, dielectric as the reference, none of
 *                          them normalised), next.time = the ray's time, next.tmax = +inf.
 *     RTOW_STEP_ABSORBED   a hit whose scatter returns nothing (the Lambertian near-zero direction): hit is filled,
 *                          atten = 0, next = the dead ray.
 *   buffers    d_rays, d_next: rtow_ray_t[n], 16-byte aligned; d_ids: uint32_t[n][2], 8-byte aligned, or NULL; d_atten:
 *              double[n][3], 8-byte aligned; d_status: int32_t[n], 4-byte aligned; d_hits: rtow_hit_t[n], 8-byte aligned,
 *              or NULL (no records are written).  All DEVICE pointers.  All n entries of every non-NULL output are
 *              written and nothing beyond n.  d_next == d_rays is allowed (ray i is read before next i is written, and no
 *              other index is touched); any other overlap is undefined.
 *   precision  RTOW_F64_STRICT: hit is bit-identical to strict rtow_intersect on the same ray and kernel, next to the
 *                               next segment of the oracle's path, atten on a miss to the sky strict rtow_radiance adds;
 *              RTOW_F64_FAST:   the fast build's walks and contracted arithmetic;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     as rtow_intersect_device: the same resolution, fallbacks, residency rules (RTOW_ENOSCENE after a lean
 *              upload) and kernel_used; RTOW_KERNEL_REFTREE is strict only.  GRID walks the direction with -0.0 replaced
 *              by +0.0; the hit record and the scatter use the caller's direction.
 * Enqueued on hip_stream with the ordering rule of rtow_intersect_device; returns without synchronising unless stats !=
 * NULL, which synchronises and fills segments = n_rays, prim_tests, node_tests, kernel_ms, total_ms, kernel_used.
 * Errors: those of rtow_radiance_device, and RTOW_EINVAL for bounce < 0, a NULL d_next, d_atten or d_status with
 * n_rays > 0, or a misaligned buffer.  n_rays == 0 returns RTOW_OK and launches nothing.  One call in flight per context.
 * The render path is not involved: the profile ring and the dropped-sample word are untouched, and a render, an
 * rtow_intersect or an rtow_radiance after any number of steps is bit-identical to one without them. */
typedef struct rtow_step_params_t {  /* 16 B */
  uint64_t seed;          /* Philox key, as rtow_config_t::seed */
  int32_t bounce;         /* >= 0: this segment's index on its path; the scatter draws request 1 + bounce */
  uint32_t sample_first;  /* added (mod 2^32) to every ray's sample index, as in rtow_radiance */
} rtow_step_params_t;

#define RTOW_STEP_MISS 0
#define RTOW_STEP_SCATTERED 1
#define RTOW_STEP_ABSORBED 2
#define RTOW_STEP_SKIPPED 3

int rtow_path_step_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_step_params_t *params,
                          const void *d_rays, int64_t n_rays, const void *d_ids /* uint32_t[n_rays][2] or NULL */,
                          void *d_next /* rtow_ray_t[n_rays]; may equal d_rays */, void *d_atten /* double[n_rays][3] */,
                          void *d_status /* int32_t[n_rays] */, void *d_hits /* rtow_hit_t[n_rays] or NULL */,
                          void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous.  hits may be NULL. */
int rtow_path_step(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_step_params_t *params,
                   const rtow_ray_t *rays, int64_t n_rays, const uint32_t *ids, rtow_ray_t *next, double *atten,
                   int32_t *status, rtow_hit_t *hits, rtow_stats_t *stats);

/* ---- ambient queries: hemisphere visibility at caller surface points ----------------------------------------------------
 * "How much of the hemisphere above this surface point is open, which way is it open, and how much sky arrives through
 * it?" — ambient occlusion, bent normals and sky-light baking for lightmap texels and probes, and the direct sky term for
 * callers who drive their own bounces with rtow_path_step.  For every point the kernel draws `samples` cosine-weighted
 * directions over the hemisphere of the normal from the point's Philox identity, asks rtow_occluded's question of each,
 * and adds up the samples that are not occluded.  The n x samples rays (64 B each) a caller of rtow_occluded would
 * generate, write and fold never reach memory, unless they are asked for (d_rays_out).
 *
 *   identity   sample j of point i draws Philox REQUEST 0 of (pixel, sample) = (ids[i][0], ids[i][1] + sample_first + j),
 *              the sums mod 2^32; without ids (NULL) of (i, sample_first + j).  Request 0 is the camera's (jitter, shutter
 *              time, lens point); no other query draws it.
 *   direction  (px, py) = the lens point of that block (lens_from_block, csrc/rtow_trace_rng.h: uniform on the unit disk);
 *              pz = sqrt(max(1 - (px px + py py), 0)) — the clamp acts: with the sampler's sine polynomial (error 7e-9)
 *              px px + py py reaches 1 + 1.3e-8 at the largest radii; n = normal / sqrt(normal . normal); (t, b, n) the
 *              branch-free orthonormal frame of Duff et al., "Building an orthonormal basis, revisited" (JCGT 6(1), 2017):
 *              s = copysign(1, n.z), a = -1 / (s + n.z), c = n.x n.y a, t = (1 + s n.x^2 a, s c, -s n.x),
 *              b = (c, s + n.y^2 a, -n.y);  d = (t px + b py) + n pz, NOT renormalised: cosine-weighted over the hemisphere
 *              of n, |d| = 1 to rounding and up to 1 + 1e-8 where the clamp acted — so max_dist is a distance to that
 *              relative accuracy.  The operand order of every expression is written once, in csrc/rtow_ambient.h.
 *   visibility the ray (point, d, time, tmax = max_dist) is occluded exactly when rtow_occluded of the same precision and
 *              kernel says so: some primitive's hit test accepts a t in [0.001, max_dist]; triangles are hit only where
 *              det >= 1e-6, as everywhere else in the library.  The GRID walk takes d as it is, as rtow_occluded's does
 *              (a -0.0 component steps the way its reciprocal points; the answer is the same as for +0.0).  tmin = 0.001
 *              is the library's: a caller who needs a larger offset moves the point.
 *   sums       for each sample that is NOT occluded, in sample order, by one lane, starting from +0.0:  open += 1;
 *              bent += d;  sky += the reference's background for d (src/render.cpp:122-128: what rtow_path_step reports
 *              as the attenuation of a MISS).  The caller divides: open / samples is the cosine-weighted visibility
 *              (1 - ambient occlusion), bent / |bent| the bent normal, sky / samples the irradiance of the sky over pi.
 *              A call with samples = k equals the in-order sum of k one-sample calls with sample_first + j, bit for bit
 *              in both builds; no result depends on the batch's shape or on scheduling.
 *   skipped    a point whose normal . normal (in binary64) is 0, subnormal (below 2^-1022: a length under about 1.5e-154),
 *              NaN or infinite (a length over about 1.3e154), or whose max_dist is NaN or below 0.001, does no walk: a
 *              subnormal normal . normal has too few bits left to normalise by.  All eight doubles of its record are +0.0
 *              (samples included), and its rays_out slots hold the dead ray of rtow_path_step (every field 0, tmax = -1).
 *   d_rays_out optional (NULL: nothing is exported): rtow_ray_t[n][samples], point-major — exactly the rays the walks took
 *              (origin = point, direction = d, time, tmax = max_dist).  rtow_occluded on them and the sums above ARE the
 *              record; a caller can also reuse the directions.
 *   buffers    d_points: rtow_surface_point_t[n]; d_out: rtow_ambient_t[n]; d_rays_out — all 16-byte aligned; d_ids:
 *              uint32_t[n][2], 8-byte aligned, or NULL.  All DEVICE pointers.  Nothing is written beyond n records and
 *              n x samples rays.
 *   precision  RTOW_F64_STRICT: bit-identical to the definition above evaluated in IEEE binary64 without contraction, in
 *                               the operand order of csrc/rtow_ambient.h, under BRUTE, BVH, GRID and BVH4 (for time in
 *                               [0, 1]) and under REFTREE against its own closest hit, with either builder;
 *              RTOW_F64_FAST:   the same expressions contracted, with the fast build's sqrt, rcp and div, and the fast
 *                               build's any-hit walks (the band of rtow_occluded_device);
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     as rtow_occluded_device: the same resolution, fallbacks, residency rules (RTOW_ENOSCENE after a lean
 *              upload) and kernel_used; RTOW_KERNEL_REFTREE is strict only.
 * Enqueued on hip_stream with the ordering rule of rtow_intersect_device; returns without synchronising unless stats !=
 * NULL, which synchronises and fills samples = segments = n * params->samples, prim_tests, node_tests, kernel_ms,
 * total_ms, kernel_used.
 * Errors: those of rtow_radiance_device, and RTOW_EINVAL for samples outside [1, RTOW_MAX_AMBIENT_SAMPLES], for
 * n * samples > 2^31 - 64 when d_rays_out is given, for points, results or rays that are not 16-byte aligned and ids that
 * are not 8-byte aligned.  n == 0 returns RTOW_OK and launches nothing.  One call in flight per context.  The render path
 * is not involved: the profile ring and the dropped-sample word are untouched, and a render or any other query after any
 * number of ambient queries is bit-identical to one without them. */
typedef struct rtow_surface_point_t { /* 64 B, 16-byte aligned: the layout of rtow_ray_t */
  double point[3];
  double time;      /* shutter time of the moving spheres, as in the ray queries */
  double normal[3]; /* need not be unit length (a length outside [1.5e-154, 1.3e154] is skipped) */
  double max_dist;  /* occluders count within [0.001, max_dist]; +inf: unbounded */
} rtow_surface_point_t;

typedef struct rtow_ambient_params_t { /* 16 B */
  uint64_t seed;          /* Philox key, as rtow_config_t::seed */
  int32_t samples;        /* 1 .. RTOW_MAX_AMBIENT_SAMPLES per point */
  uint32_t sample_first;  /* added (mod 2^32) to every point's first sample index */
} rtow_ambient_params_t;

typedef struct rtow_ambient_t { /* 64 B, 16-byte aligned: four 16-byte stores per point */
  double open;     /* number of samples that are not occluded */
  double bent[3];  /* sum of their directions */
  double sky[3];   /* sum of the reference's sky colour over their directions */
  double samples;  /* samples taken: params->samples, or 0 for a skipped point */
} rtow_ambient_t;

#define RTOW_MAX_AMBIENT_SAMPLES 65536

int rtow_ambient_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_ambient_params_t *params,
                        const void *d_points /* rtow_surface_point_t[n] */, int64_t n,
                        const void *d_ids /* uint32_t[n][2] or NULL */, void *d_out /* rtow_ambient_t[n] */,
                        void *d_rays_out /* rtow_ray_t[n][samples] or NULL */, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous.  ids and rays_out
 * may be NULL. */
int rtow_ambient(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_ambient_params_t *params,
                 const rtow_surface_point_t *points, int64_t n, const uint32_t *ids, rtow_ambient_t *out,
                 rtow_ray_t *rays_out, rtow_stats_t *stats);

/* ---- swept-sphere (sphere cast) queries ---------------------------------------------------------------------------------
 * "Where does a ball travelling along this segment first touch the scene, and what does it touch?" — a camera that must
 * not clip through geometry, a character or particle with a size, a thick ray, continuous collision, clearance along a path.
 *
 * Definition.  The geometry is that of rtow_closest_point: the device's records, the sphere SURFACE | |p - c| - R | with
 * R = sqrt(|r^2|), a moving sphere's centre at the query's `time`.  A hollow (negative-radius) sphere is the same surface,
 * so a sphere cast inside a large sphere touches its inner side.  For a query (o, d, time, tmax, rho) write
 * p(t) = o + d t and D(x, c) for the distance from x to primitive c.  Primitive c answers with the smallest t in
 * [0, tmax] with D(p(t), c) <= rho — none when the sphere never comes that close; t is in units of |d|.  The scene's
 * answer is the minimum over the primitives by (t, insertion index): the lowest index wins an exact tie (the tie rule of
 * rtow_first_hits), so the strict answer does not depend on kernel, builder or schedule.
 *
 * Per-primitive formulas (csrc/rtow_sweep_walks.h; written once, in a fixed operation order; tests/sweep_ref.py mirrors
 * them).  Every root of |w + d t| = r is taken through the perpendicular q = w + d t0, t0 = -(w.d) / (d.d), as
 * t0 -+ sqrt((r^2 - q.q) / d.d): well conditioned for a far origin and for a sweep nearly parallel to an edge.
 *   start overlap  (all primitives) the formulas of rtow_closest_point at o give a distance <= rho: t = 0 and
 *                  start_overlap = 1.  In the strict build start_overlap == 1 exactly when strict
 *                  rtow_closest_point(o, time, max_dist = rho) reports a hit.
 *                  Otherwise no piece asks again whether the sweep starts outside it: over the reals the failed
 *                  overlap test says so, and a second test in other arithmetic would disagree with it on a shell a few
 *                  ulps thick — exactly where a sweep starts that continues from the centre of an earlier contact.  Every
 *                  near root is clamped at 0 instead: a start that a piece's own arithmetic puts inside it answers t = 0
 *                  with start_overlap = 0, a contact at rho within the band like any other.
 *   sphere         with oc = o - c, L2 = oc.oc, h = oc.d: from the outer side (L2 >= |r^2|) the near root of
 *                  |p - c| = R + rho, a hit iff the perpendicular is no longer than R + rho and h < 0 — a tangent pass
 *                  touches: the contact set is closed; from the inner side (L2 < |r^2|, hence R > rho) the far root of
 *                  |p - c| = R - rho, which exists for every direction (a negative term under its root is rounding: 0).
 *   triangle       the minimum over the accepted candidates of the pieces of the Minkowski sum:
 *                  face — only when n.n > 0 and the centre approaches the plane: where the centre reaches the offset plane
 *                    on its own side, t = max(|n.(o - a)| - rho |n|, 0) / |n.d|, accepted when the Gram-form barycentrics
 *                    of p(t) - a lie inside (sn, tn in [0, n.n], sn + tn <= n.n, as in rtow_closest_point);
 *                  three edges — for each edge with e.e > 0 the near root of the infinite cylinder of radius rho about the
 *                    edge line, accepted when the sweep approaches its axis and the axial parameter at contact lies in
 *                    [0, e.e];
 *                  three vertices — the near root of the sphere of radius rho about each vertex, when the sweep
 *                    approaches it.
 *                  (A start inside a piece that the overlap test did not see lies beyond a cap or beside the prism, where
 *                  the axial or barycentric test rejects it, or in the shell.)
 *                  Exact over the reals: the sum is the union of a prism and three capsules; the first entry into a union
 *                  is the minimum of the first entries into its convex parts; a lateral entry into the prism, or an entry
 *                  through a cylinder cap, lies inside a capsule or a vertex sphere; every accepted candidate is a point
 *                  of the union.  A degenerate triangle answers as its edges and vertices do.  No division is unguarded and
 *                  no field is ever NaN for a finite query.  rho = 0 is allowed: a two-sided ray against the surfaces,
 *                  with no determinant cut and t from 0.
 *   acceptance     a candidate is accepted when t <= bound, inclusive; the bound starts at tmax and shrinks to the best t;
 *                  every member of a tie at the bound is still visited.
 *   skipped        the miss record and no walk when: o, time, d, tmax or radius is NaN; radius is negative or infinite;
 *                  tmax is negative; d.d is 0 or infinite; o or time is infinite.  (pad_ is not read.)  tmax = +inf is
 *                  unbounded.
 *   time           results are independent of the kernel for time in [0, 1] only, as for every other query.
 *
 *   precision  RTOW_F64_STRICT: the whole record is bit-identical to the definition evaluated by those formulas in IEEE
 *                               binary64 in their written order, under BRUTE, BVH, BVH4 and AUTO, with either builder and
 *                               after a refit;
 *              RTOW_F64_FAST:   the same formulas contracted (FMA) with the fast build's square root and reciprocal.  Its
 *                               promise is semantic, with the band B(c) = 96 u S(c), u = 2^-53, S(c) = |o|_1 + |t d|_1 +
 *                               rho + the magnitudes of primitive c (|a|_1 + |e1|_1 + |e2|_1; |c|_1 + R; |c0|_1 +
 *                               |time (c1 - c0)|_1 + R), t the reported t (tmax on a miss):
 *                                 a hit on c* at t <= tmax: | D(centre, c*) - rho | <= B(c*) — on a start overlap t == 0 and
 *                                   D(o, c*) <= rho + B(c*); dist and point meet rtow_closest_point's two point clauses at
 *                                   centre; and no primitive was passed through on the way: the distance from the segment
 *                                   [o, centre] to every primitive c is >= rho - B(c);
 *                                 a miss: the distance from the segment [o, p(tmax)] to every c is >= rho - B(c).
 *                               Where a primitive's segment distance is within its band of rho either answer is allowed.
 *                               The strict build meets the same with 48 u (tests/sweep_ref.py counts the roundings);
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *   kernel     BRUTE, BVH and BVH4 run their own walks (ray walks against boxes inflated by rho); GRID has no sweep walk
 *              and is answered by BVH (kernel_used says BVH); AUTO takes BVH4, else BVH, else BRUTE; the fallbacks and
 *              RTOW_ENOSCENE rules are rtow_closest_point's.  RTOW_KERNEL_REFTREE: RTOW_EINVAL.
 * dist and point are exactly what the formulas of rtow_closest_point compute at centre for the winning primitive: the
 * contact normal is centre - point, and a caller who wants it unit-length divides by dist.  d_queries / d_hits are DEVICE
 * pointers, both 16-byte aligned; nothing beyond n is written.  Stream ordering, stats (segments = n, prim_tests,
 * node_tests, kernel_ms, total_ms, kernel_used) and errors are those of rtow_closest_point_device.  n == 0 launches
 * nothing.  One call in flight per context; the render path (profile ring, dropped-sample word) is not involved. */
typedef struct rtow_sweep_t {      /* 80 B, 16-byte aligned: five 16-byte loads */
  double origin[3]; double time;
  double direction[3]; double tmax;
  double radius; double pad_;
} rtow_sweep_t;

typedef struct rtow_sweep_hit_t {  /* 80 B, 16-byte aligned: five 16-byte stores */
  double t;          /* +inf on a miss */
  double dist;       /* closest-point distance from centre to the primitive: ~radius at a contact, below it on a start
                        overlap (radius - dist is the penetration depth); +inf on a miss */
  double centre[3];  /* origin + direction*t; 0 on a miss */
  double point[3];   /* the closest point of that primitive to centre: the contact point; 0 on a miss */
  int32_t prim, kind, material;   /* as rtow_point_hit_t; -1 on a miss */
  int32_t start_overlap;          /* 1 when t == 0 because the sphere already touches at the origin */
} rtow_sweep_hit_t;

int rtow_sweep_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_queries, int64_t n,
                      void *d_hits, void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_sweep(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_sweep_t *queries, int64_t n,
               rtow_sweep_hit_t *hits, rtow_stats_t *stats);

/* ---- box overlap: which primitives are inside this region, and how many ----------------------------------------------------
 * Per query a closed axis-aligned box [lo, hi], a shutter time and a first insertion index min_prim.  O is the set of
 * primitives with insertion index >= min_prim (a negative min_prim acts as 0) whose geometry overlaps the box.  The
 * geometry is that of rtow_closest_point and rtow_sweep, the device's records: a triangle is the closed triangle a, a + e1,
 * a + e2 (a zero-area triangle its segment or point); a sphere or moving sphere is its SURFACE, centre taken at `time`
 * (c0 + time (c1 - c0)), radius^2 = |r2|: it overlaps the box iff dmin^2 <= R^2 <= dmax^2, dmin the distance from the
 * centre to the box and dmax that to the box's farthest corner, so a box wholly inside a sphere does not overlap it (the
 * hollow sphere the closest-point query and the sweep see).  Touching counts: every comparison is inclusive.
 *
 *   counts[i]  |O|, uncapped.
 *   ids[i][j]  for j < min(|O|, max_ids) the lowest insertion indices of O, ascending; the remaining slots -1.  Every slot
 *              of every query is written; nothing is written beyond n.  d_ids may be NULL (counts only: the list is not
 *              kept); d_counts is required.
 *   max_ids    1 .. RTOW_MAX_OVERLAP_IDS, checked where rtow_nearest checks k: outside that range RTOW_EINVAL.
 *   paging     while counts[i] > max_ids, the same query with min_prim = ids[i][max_ids - 1] + 1 continues the list: the
 *              pages are disjoint, ascending, and together all of O (Context.overlap_all does this).
 *   skipped    count 0, ids -1 and no walk when lo, hi or time holds a NaN or an infinity, or lo > hi in a component.
 *              (pad_ is not read.)  lo == hi in one, two or three components is a rectangle, a segment, a point.
 *   time       results are independent of the kernel for time in [0, 1] only, as for every other query.
 *
 * The predicate (csrc/rtow_overlap_walks.h; written once, in a fixed operation order, on the inputs as given;
 * tests/overlap_ref.py mirrors it) is a separating-axis test with no division, square root or reciprocal:
 *   sphere     per component near = max(max(lo - s, s - hi), 0), far = max(s - lo, hi - s), s the centre; dmin^2 and
 *              dmax^2 the sums of their squares, (x + y) + z; overlap iff dmin^2 <= |r2| and |r2| <= dmax^2.
 *   triangle   v1 = a + e1, v2 = a + e2, f = e2 - e1; thirteen axes: the three box normals (min(a, v1, v2) > hi or
 *              max(a, v1, v2) < lo separates), the stored n (n.a against the box's interval [sum_k min(n_k lo_k, n_k hi_k),
 *              sum_k max(n_k lo_k, n_k hi_k)]) and the nine edge x box-axis products, whose components are copies of the
 *              edge's (e1 with vertices a, v2; e2 and f with a, v1), each against the box's interval on that axis.
 *
 *   precision  RTOW_F64_STRICT: counts and ids are bit-identical to that predicate evaluated in IEEE binary64 in its
 *                               written order, under BRUTE, BVH, BVH4 and AUTO, with either builder and after a refit;
 *              RTOW_F64_FAST:   the same predicate with FMA contraction; not promised to be the same under every kernel;
 *              RTOW_F32:        refused (RTOW_EINVAL).
 *              Both against exact arithmetic: for an axis L, s_L is the exact signed gap (triangle: the greater of
 *              "least projection of the exact vertices a, a + e1, a + e2 minus the box's greatest" and "the box's least
 *              minus their greatest", with the exact e1 x e2 for the normal; sphere: dmin^2 - R^2 and R^2 - dmax^2) and E_L
 *              the sum of the magnitudes of the monomials of s_L expanded in the inputs as given — the record's fields,
 *              lo, hi, time — taking of a min or max the branch the exact values select (the larger sum on an exact
 *              tie: the two vertices of an edge project alike across it).  With u = 2^-53 a pair is DECIDED when some axis has s_L > K u E_L (it
 *              is not reported) or every axis with L != 0 has s_L < -K u E_L (it is reported); any other pair may go
 *              either way.  K = 10 for the strict build: no monomial of a gap passes more than 9 roundings (the moving
 *              sphere: 2 in the centre, 1 in the difference, doubled by the square, 1 for the square and 2 for the sums;
 *              a fixed sphere 5; the normal axis 5: 2 in the stored n, the product, two sums; a cross axis 4; a box
 *              normal 1), and one more covers the terms of second order.  K = 20 for the fast build.
 *              Where every intermediate is exactly representable — small-integer or dyadic coordinates — both builds
 *              give the exact closed-set answer, touching at a face, along an edge and at a vertex included.
 *   kernel     BRUTE, BVH and BVH4 run their own walks (a node is entered iff its box meets the query box inflated by
 *              the point walks' slack, inclusive); GRID has no overlap walk and is answered by BVH (kernel_used says
 *              BVH); AUTO takes BVH4, else BVH, else BRUTE and never fails on a resident scene; the fallbacks and
 *              RTOW_ENOSCENE rules are rtow_closest_point's.  RTOW_KERNEL_REFTREE: RTOW_EINVAL.
 * d_queries (16-byte aligned), d_counts and d_ids (4-byte aligned) are DEVICE pointers.  Stream ordering, stats
 * (segments = n, prim_tests, node_tests, kernel_ms, total_ms, kernel_used) and errors are those of
 * rtow_closest_point_device.  n == 0 launches nothing.  One call in flight per context. */
typedef struct rtow_box_query_t {   /* 64 B, 16-byte aligned in device memory: four 16-byte loads */
  double lo[3], hi[3];              /* the closed box [lo, hi] */
  double time;                      /* moving-sphere centre c0 + time*(c1-c0), as in the point queries */
  int32_t min_prim;                 /* only primitives with insertion index >= min_prim take part; < 0 acts as 0 */
  int32_t pad_;
} rtow_box_query_t;
#define RTOW_MAX_OVERLAP_IDS 8
int rtow_overlap_device(rtow_ctx *ctx, int32_t precision, int32_t kernel, const void *d_queries, int64_t n,
                        int32_t max_ids, void *d_counts /* int32_t[n] */, void *d_ids /* int32_t[n][max_ids] or NULL */,
                        void *hip_stream, rtow_stats_t *stats);
/* The same from and to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_overlap(rtow_ctx *ctx, int32_t precision, int32_t kernel, const rtow_box_query_t *queries, int64_t n,
                 int32_t max_ids, int32_t *counts, int32_t *ids /* or NULL */, rtow_stats_t *stats);

/* ---- the camera stage: primaries of the resident camera, first-hit guide buffers ----------------------------------------
 * The one piece of the render the queries above leave out: Camera::get_ray (src/render.cpp:158-159,
 * src/common-model.cpp:156-167) for the camera of the scene resident in ctx (after the last upload or refit), fed from
 * request 0 of (pixel, sample) — pixel jitter, shutter time and lens point exactly as the render draws them.
 *
 * Both calls read `cfg` as rtow_render_device does: image_width / image_height and seed; rank / nranks / tile_rows select
 * this rank's rows (ascending, rtow_local_row_list); the sample set is the one a render of cfg traces — samples
 * [0, spp_eff) with spp_eff = samples_per_pixel / nstreams * nstreams when stream_count == 0, otherwise the samples of
 * streams [stream_first, stream_first + stream_count), each stream samples_per_pixel / nstreams long.  max_child_rays and
 * accumulate are ignored.  precision: RTOW_F64_STRICT or RTOW_F64_FAST; RTOW_F32 is refused (RTOW_EINVAL).  Stream
 * ordering, errors, RTOW_ENOSCENE and "nothing to do launches nothing" follow rtow_intersect_device.  The render path is
 * not involved: the profile ring, the dropped-sample word and the workspace are untouched, and a render after any number
 * of these calls is bit-identical to one without them.
 *
 * rtow_camera_rays*: n = local_rows * image_width * samples rays (rtow_camera_ray_count; must not exceed 2^31 - 64),
 * pixel-major over the rank's rows, a pixel's samples ascending.  ids[i] = (global row-major pixel index, sample index):
 * the Philox identity rtow_radiance takes, so radiance(camera_rays(cfg), ids, seed, max_child_rays) added per pixel in
 * sample order IS the render (bit for bit in the strict build with nstreams == 1).  tmax = +inf.
 *   RTOW_F64_STRICT: origin, direction and time are bit-identical to the reference's get_ray on the oracle's draws;
 *   RTOW_F64_FAST:   the fast render's camera arithmetic (contracted; u and v multiply by 1 / (W - 1) and 1 / (H - 1)).
 * The kernel reads the camera alone: cfg->kernel is ignored except that an unknown value is RTOW_EINVAL, and the call
 * works after the lean upload of rtow_render too.  d_rays: rtow_ray_t[n], DEVICE memory, 16-byte aligned; d_ids:
 * uint32_t[n][2], DEVICE memory, 8-byte aligned, or NULL (no ids are written).  Returns without synchronising.
 *
 * rtow_guides*: what a denoiser takes beside the beauty image, with the render's own jitter, lens and shutter samples, so
 * that depth of field and motion blur agree between the guides and the image.  Per pixel, SUMS over the pixel's samples
 * (the caller divides: hits / samples is coverage, depth / hits the mean distance over the hits), added by one lane in
 * sample order from +0.0.  Per sample, with the primary (o, d, time) and its closest hit over [0.001, inf):
 *   hit   albedo += the attenuation the reference's scatter returns: the albedo (Lambertian, Metal), (1, 1, 1) (Dielectric);
 *         normal += the unit shading normal: a sphere's Hit::normal (normalize(p - c), facing the ray), a triangle's
 *                   n / sqrt(n . n) with n = e1 x e2;
 *         depth  += t * sqrt(d . d), the distance from the ray origin;   hits += 1;
 *   miss  albedo += the reference's sky for d (ray_color's miss branch); normal, depth and hits add nothing.
 * The operand order of every expression is written in csrc/rtow_guides.h; RTOW_F64_STRICT evaluates it without
 * contraction (bit-identical to that order in IEEE binary64, under every kernel, with either builder and for every
 * partition of the image), RTOW_F64_FAST contracted with the fast build's sqrt, rcp and div.  No result is NaN for a
 * finite scene.  cfg->kernel: resolution, fallbacks, residency rules (RTOW_ENOSCENE after a lean upload that did not
 * build the strategy's structures) and kernel_used as rtow_intersect_device; RTOW_KERNEL_REFTREE is strict only.
 * d_guides: rtow_guide_t[local_rows * image_width], DEVICE memory, 16-byte aligned, row-major over this rank's rows.
 * With stats it synchronises and fills samples = segments = pixels * samples, prim_tests, node_tests, kernel_ms,
 * total_ms, kernel_used, local_rows. */
typedef struct rtow_guide_t { /* 64 B: four 16-byte stores per pixel */
  double albedo[3];
  double normal[3];
  double depth;
  double hits;
} rtow_guide_t;

int rtow_camera_rays_device(rtow_ctx *ctx, const rtow_config_t *cfg, void *d_rays /* rtow_ray_t[n] */,
                            void *d_ids /* uint32_t[n][2] (pixel, sample) or NULL */, void *hip_stream);
/* The same to host memory (device staging owned by the context, the null stream); synchronous.  ids may be NULL. */
int rtow_camera_rays(rtow_ctx *ctx, const rtow_config_t *cfg, rtow_ray_t *rays, uint32_t *ids);
/* n of the two calls above, or a negative RTOW_E* code for an invalid cfg — pure host arithmetic, usable without a GPU. */
int64_t rtow_camera_ray_count(const rtow_config_t *cfg);

int rtow_guides_device(rtow_ctx *ctx, const rtow_config_t *cfg, void *d_guides /* rtow_guide_t[local_rows * W] */,
                       void *hip_stream, rtow_stats_t *stats);
/* The same to host memory (device staging owned by the context, the null stream); synchronous. */
int rtow_guides(rtow_ctx *ctx, const rtow_config_t *cfg, rtow_guide_t *guides, rtow_stats_t *stats);

/* ---- in-place refit of the resident scene (moving geometry) ---------------------------------------------------------
 * Replace the geometry, materials and camera of the scene resident in ctx, keeping its trees' topology: the node
 * structure, leaf membership and leaf order of the binary and 4-wide BVHs stay as built; records, boxes and planes are
 * recomputed on the GPU (csrc/rtow_refit.hip) by the host builder's rules, the grid is rebuilt (present afterwards
 * exactly when a fresh upload of `scene` would build it).  Only the images the resident scene holds are refreshed (after
 * the lean upload of rtow_render*, those its kernel reads).  An unchanged refit right after a host-builder upload leaves
 * every image byte-identical.
 *   may change   every sphere, moving sphere and triangle; material indices and records; the camera (t0 / t1 included)
 *   must keep    n_spheres, n_moving, n_triangles, n_materials, n_prims, and prim_kind / prim_index (identical, or
 *                absent in both); anything else is RTOW_EINVAL with the resident scene untouched
 * Ordering: as rtow_scene_upload (waits for earlier device work, queues on the null stream, later renders and queries on
 * any stream see the new scene).  Hit `prim` ids keep naming primitives in insertion order.  Culling quality degrades
 * as the geometry moves away from the uploaded shape (rtow_refit_info_t::bvh_area_ratio); re-upload when it has.
 * Errors: RTOW_EINVAL (NULL ctx or scene, an invalid scene, a shape mismatch), RTOW_ENOSCENE without a resident scene. */
int rtow_scene_refit(rtow_ctx *ctx, const rtow_scene_t *scene);

typedef struct rtow_refit_info_t {
  int32_t refits;          /* refits since the last rtow_scene_upload / rtow_render upload */
  int32_t grid_resident;   /* the grid image exists after the last refit (it is rebuilt) */
  double refit_ms;         /* host wall time of the last rtow_scene_refit call */
  double device_ms;        /* device time of the last refit's kernels and copies (HIP events) */
  double bvh_area_ratio;   /* sum of the binary BVH's inner-node half-areas / root half-area for the current geometry, over
                              the same sum for the geometry of the upload.  1.0 = as built, and before any refit; grows
                              as the tree degrades.  0 when no binary BVH is resident. */
} rtow_refit_info_t;
/* Facts about the refits since the last upload; synchronises.  RTOW_ENOSCENE without a scene. */
int rtow_refit_info(rtow_ctx *ctx, rtow_refit_info_t *out);

/* Convenience: upload + render + copy this rank's rows to host memory.
 * Lean upload: rtow_render / rtow_render_rgb8 know their config and build only the structures ITS kernel reads
 * (the cover scene through the grid kernel needs no BVH, no 4-wide image, no binary32 images).  The scene they
 * leave resident is therefore partial: a later rtow_render_device with another kernel or precision is refused with
 * RTOW_ENOSCENE until rtow_scene_upload (which builds everything) has run. */
int rtow_render(rtow_ctx *ctx, const rtow_scene_t *scene, const rtow_config_t *cfg,
                double *rgb_sums_host, rtow_stats_t *stats);

/* Convenience: upload + render + write_color on the device + copy this rank's rows as 8-bit
 * RGB (rows*W*3 bytes) to host memory — the payload of a binary P6 PPM. */
int rtow_render_rgb8(rtow_ctx *ctx, const rtow_scene_t *scene, const rtow_config_t *cfg,
                     unsigned char *rgb8_host, rtow_stats_t *stats);

/* One frame over several HIP devices from ONE process (replaces the reference's thread fan-out and
 * in-order sum, src/render.cpp:169-180): one host thread + context per entry of `device_ids`, strips of
 * cfg->tile_rows rows dealt round-robin (cfg->rank / nranks are ignored: rank = position in the list),
 * then with use_rccl != 0 ONE ncclGather (RCCL over xGMI; librccl.so is loaded on demand) of the strip
 * buffers to the first device and ONE device-to-host copy, with use_rccl == 0 one copy per device.
 * `rgb_sums_host`: image_height*image_width*3 doubles, row-major from the top, the radiance sums of
 * the whole frame — identical, bit for bit, to a one-device rtow_render of the same config.  RCCL rejects
 * a device listed twice; use_rccl == 0 accepts it (tests of the partition on a one-GPU machine). */
int rtow_render_multi(int32_t n_devices, const int32_t *device_ids, const rtow_scene_t *scene,
                      const rtow_config_t *cfg, double *rgb_sums_host, rtow_stats_t *stats, int32_t use_rccl);

/* The same as a persistent handle, for more than one frame: rtow_render_multi pays for its contexts,
 * streams, buffers, worker threads and — by far the largest item — the RCCL communicator on every call
 * (it is create + upload + render + destroy).  The handle owns all of them; rtow_multi_upload builds
 * the scene's acceleration structures once per device (concurrently); rtow_multi_render is then one
 * trace launch per device, the one ncclGather enqueued behind them on the same streams, a small kernel on the
 * first device that puts the strips' rows in place, and ONE device-to-host copy straight into the caller's buffer
 * (no host pass over the pixels).  One call in flight per handle.
 * rtow_multi_render_rgb8: the same with write_color run by the rank that owns the pixel (the fused reduce of
 * rtow_render_device_rgb8), so the gather and the copy move 3 bytes per pixel instead of 24; `rgb8_host` receives
 * image_height*image_width*3 bytes, equal to a one-device rtow_render_rgb8 of the same config.
 * If a rank cannot enqueue its side of the gather, every communicator is aborted (ncclCommAbort) before anything
 * is waited for, the call returns RTOW_EHIP and the handle refuses further frames: an error is a code, never a hang.
 * rtow_multi_build_info reports the first device's build (every device builds the same structures).
 * A frame is ONE hand-off to the worker threads (trace launch, a meeting of the workers, each rank's side of the
 * gather), the placement kernel only when there is more than one rank, one asynchronous copy into the caller's
 * buffer and ONE wait, on the first device's stream (it is ordered behind every other rank's queue by events).
 * rtow_multi_frame_breakdown: where the last successful frame's time went, RTOW_MULTI_BREAKDOWN_FIELDS doubles in
 * milliseconds indexed by RTOW_MB_* (host clock around the call's stages; HIP events on the first device's stream
 * for the device side); returns the number of fields written. */
typedef struct rtow_multi rtow_multi;
enum {
  RTOW_MB_TOTAL = 0,           /* entry to return of rtow_multi_render* (host clock) */
  RTOW_MB_HANDOFF_ENQUEUE = 1, /* buffers, the hand-off to the workers, until every rank has queued its frame */
  RTOW_MB_PLACE_ENQUEUE = 2,   /* error collection, stream-wait events, the placement kernel's launch */
  RTOW_MB_WAIT_AND_COPY = 3,   /* queueing the device-to-host copy + the one wait (device work still running included) */
  RTOW_MB_WAIT_ONLY = 4,       /* RTOW_MULTI_D2H=blocking only: the wait before the blocking copy */
  RTOW_MB_DEV_TRACE = 5,       /* first device: trace + reduce (+ write_color), events */
  RTOW_MB_DEV_GATHER = 6,      /* first device: the gather (or the strips' copy), events */
  RTOW_MB_DEV_PLACE_COPY = 7,  /* first device: waits for the other ranks, placement kernel, device-to-host copy, events */
  RTOW_MULTI_BREAKDOWN_FIELDS = 8
};
int rtow_multi_create(int32_t n_devices, const int32_t *device_ids, int32_t use_rccl, rtow_multi **out);
int rtow_multi_set_builder(rtow_multi *m, int32_t builder);
int rtow_multi_upload(rtow_multi *m, const rtow_scene_t *scene);
int rtow_multi_build_info(rtow_multi *m, rtow_build_info_t *out);
int rtow_multi_render(rtow_multi *m, const rtow_config_t *cfg, double *rgb_sums_host, rtow_stats_t *stats);
int rtow_multi_render_rgb8(rtow_multi *m, const rtow_config_t *cfg, unsigned char *rgb8_host, rtow_stats_t *stats);
int rtow_multi_frame_breakdown(rtow_multi *m, double *out_ms, int32_t n_fields);
void rtow_multi_destroy(rtow_multi *m);

/* ---- host-side scene construction (no GPU needed) --------------------------
 * C entry points over the C++ mirror of the reference's scene-build API
 * (host/scene.h ≙ src/common-model.h, src/oo-primitives.h, src/render.h):
 * the two scene scripts of the reference's main.cpp, flattened. */
typedef struct rtow_host_config_t {
  int32_t number_of_balls_sqrt; /* src/render.h:12  */
  double aspect_ratio;          /* src/render.h:13  */
  int32_t moving_spheres;       /* src/render.h:16  */
} rtow_host_config_t;

/* lots_of_balls() (src/main.cpp:23-83): consumes the process-global mt19937
 * stream from its default seed, like the reference. */
int rtow_host_scene_cover(const rtow_host_config_t *cfg, rtow_scene_t **out);
/* foo() (src/main.cpp:85-136): triangles of the first shape of an OBJ file. */
int rtow_host_scene_obj(const rtow_host_config_t *cfg, const char *obj_path, rtow_scene_t **out);
/* The same scripts on each of the reference's scene models (it picks one at compile time): OO primitives
 * (src/oo-primitives.h — what the two entry points above use), variant primitives
 * (src/variant-primitives.h:84-113, RTWEEKEND_USE_VARIANT_PRIMITIVES) and the World of src/vmodel.h:250-253
 * (spheres only: the OBJ script has no World form).  Built by the same calls, the models flatten to the
 * same rtow_scene_t. */
#define RTOW_MODEL_OO 0
#define RTOW_MODEL_VARIANT 1
#define RTOW_MODEL_WORLD 2
int rtow_host_scene_cover_model(const rtow_host_config_t *cfg, int32_t model, rtow_scene_t **out);
int rtow_host_scene_obj_model(const rtow_host_config_t *cfg, const char *obj_path, int32_t model, rtow_scene_t **out);
void rtow_host_scene_free(rtow_scene_t *scene);
/* Reset the host scene-construction RNG to the reference's default seed. */
void rtow_host_rng_reset(void);

/* write_color + PPM (src/render.cpp:11-20,182-186): P3 text into a malloc'ed
 * buffer (`*out_text`, free with rtow_host_free). */
int rtow_host_ppm(const double *rgb_sums, int32_t width, int32_t height, int32_t spp_effective,
                  char **out_text, uint64_t *out_len);
void rtow_host_free(void *p);

/* The reference's own bounding-volume tree (src/render.cpp:73-110) over a flattened scene, as RTOW_KERNEL_REFTREE
 * walks it, built on the host (no GPU): node count, depth and the reference's "Total BVH stupid volume"
 * diagnostic (src/render.cpp:36-50,148). */
int rtow_host_reftree_info(const rtow_scene_t *scene, int32_t *n_nodes, int32_t *depth, double *stupid_volume);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_H */
