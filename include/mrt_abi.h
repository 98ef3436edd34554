/*
 * mrt_abi.h — C ABI of the MI355X-native path tracer (libmrt_hip.so).
 *
 * This is the drop-in boundary for the hot path of JaapWijnen/metal-raytracing: everything
 * `Renderer.draw(in:)` binds to `raytracingKernel` (Renderer.swift:302-329), the data contract
 * of the bridging header (ShaderTypes.h:60-107) and the acceleration-structure build
 * (Renderer.swift:184-214, Utilities.swift:29-85).  The reference has no FFI of its own; each
 * entry point below cites the reference interface it replaces.  Plain pointers and sizes only:
 * no C++ types, no torch types.  Every call returns an int status (MRT_OK == 0) and never
 * throws or aborts across the boundary; mrt_last_error() gives the thread-local message.
 *
 * Threading: one thread drives a renderer at a time (the reference drives Renderer from the
 * main thread only, Renderer.swift:284).  The library never calls back into the caller.
 */
#ifndef MRT_ABI_H
#define MRT_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRT_ABI_VERSION 3      /* 3: MRTSceneStats grew (wide_cost, wide_cost_built, refits: what a refit did to the tree); 2: (wide_layout, wide_depth), the renderer's option keys split into mrt_renderer_set_option (six host keys) and mrt_debug_renderer_set_option */

/* ---------------------------------------------------------------- status codes */
enum {
    MRT_OK = 0,
    MRT_ERR_INVALID_ARGUMENT = 1,
    MRT_ERR_NO_DEVICE = 2,      /* no HIP device / HIP runtime failure at context creation   */
    MRT_ERR_HIP = 3,            /* a HIP call failed; message carries hipGetErrorString       */
    MRT_ERR_IO = 4,             /* OBJ/MTL file could not be read                             */
    MRT_ERR_STATE = 5,          /* call order violated (e.g. render before scene commit)      */
    MRT_ERR_OUT_OF_MEMORY = 6,
    MRT_ERR_UNSUPPORTED = 7
};

/* ---------------------------------------------------------------- data contract
 * Bit layout of ShaderTypes.h:60-107.  `vector_float3` is 16-byte sized and aligned, hence the
 * explicit pad word.  Sizes and offsets are static_assert-ed in metal-raytracing_amd/csrc/abi_check.h
 * (compiled into the library) and checked through ctypes in tests/test_abi_and_host.py.         */
typedef struct { float x, y, z, _pad; } MRTFloat3;                    /* simd vector_float3     */

typedef struct {                                                      /* ShaderTypes.h:60-65    */
    MRTFloat3 position, right, up, forward;
} MRTCamera;                                                          /* 64 B                   */

typedef enum {                                                        /* ShaderTypes.h:67-74    */
    MRTLightTypeUnused = 0, MRTLightTypeSunlight = 1, MRTLightTypeSpotlight = 2,
    MRTLightTypePointlight = 3, MRTLightTypeAreaLight = 4
} MRTLightType;

typedef struct {                                                      /* ShaderTypes.h:76-87    */
    int32_t   type;            /* @0   (NSInteger on the Swift side: low 32 bits, LE)          */
    int32_t   _pad0[3];
    MRTFloat3 position;        /* @16                                                          */
    MRTFloat3 color;           /* @32                                                          */
    MRTFloat3 forward;         /* @48  area light                                              */
    MRTFloat3 right;           /* @64                                                          */
    MRTFloat3 up;              /* @80                                                          */
    float     coneAngle;       /* @96  spot light                                              */
    float     _pad1[3];
    MRTFloat3 direction;       /* @112                                                         */
} MRTLight;                                                           /* 128 B                  */

typedef struct {                                                      /* ShaderTypes.h:89-97    */
    int32_t   width, height, blocksWide;
    uint32_t  frameIndex;
    int32_t   lightCount;
    int32_t   _pad[3];
    MRTCamera camera;          /* @32                                                          */
} MRTUniforms;                                                        /* 96 B                   */

typedef struct {                                                      /* ShaderTypes.h:99-107   */
    MRTFloat3 baseColor;       /* @0  — the only field raytracingKernel reads (:269)           */
    MRTFloat3 specular;        /* @16                                                          */
    MRTFloat3 emission;        /* @32                                                          */
    float     specularExponent;/* @48                                                          */
    float     refractionIndex; /* @52                                                          */
    float     dissolve;        /* @56                                                          */
    float     _pad;
} MRTMaterial;                                                        /* 64 B                   */

/* One ray / one intersector result, as `metal::raytracing::ray` and
 * `intersector<triangle_data, instancing>::result_type` present them (Raytracing.metal:214-221,
 * :230-247).  Used by the query entry points (parity tests, brute-force cross-checks).
 * Direction components may be +0, -0 or denormal: the answer is the triangle test's either way. */
typedef struct {
    float origin[3];    float min_distance;
    float direction[3]; float max_distance;
} MRTRay;                                                             /* 32 B                   */

typedef struct {
    int32_t type;              /* 0 = none, 1 = triangle                                       */
    float   distance;
    int32_t instance_id;       /* mesh index in scene order (Renderer.swift:193-195)           */
    int32_t geometry_id;       /* submesh index within the mesh (Mesh.swift:39-48)             */
    int32_t primitive_id;      /* triangle index within the submesh                            */
    float   u, v;              /* triangle_barycentric_coord: weights of vertices 1 and 2      */
    int32_t _pad;
} MRTIntersection;                                                    /* 32 B                   */

typedef struct {
    uint64_t triangles;        /* T: triangles in the committed scene (every instance's own)   */
    uint64_t vertices;         /* V                                                            */
    uint64_t bvh_nodes;        /* nodes of the layout the rays walk: the 8-wide nodes; the binary (rope) nodes of a scene without the 8-wide
                                  layout (wide_layout = 0); two-level scenes: the nodes of the rope TLAS (the BLASes' are in scene_bytes)   */
    uint64_t bvh_leaves;       /* leaves of the binary tree after its SAH collapse, whichever layout was emitted from it (the 8-wide layout
                                  groups the same references into leaf slots of its own); two-level scenes: summed over the BLASes         */
    uint64_t scene_bytes;      /* device bytes of nodes + triangle packets + shading tables    */
    float    build_ms;         /* device time of the last mrt_scene_commit                     */
    float    sah_cost;         /* SAH cost of the emitted tree (Ct=1, Ci=1); after a refit: the build's figure x wide_cost / wide_cost_built */
    int32_t  instances;
    int32_t  max_submeshes;    /* resource-table stride (Renderer.swift:128-139)               */
    int32_t  max_leaf_tris;
    int32_t  max_depth;        /* levels of the 8-wide tree (= wide_depth); without it: depth of the binary tree in edges from its root;
                                  two-level scenes: levels of the rope TLAS                                                                */
    int32_t  wide_layout;      /* 1: the scene has the 8-wide layout and every ray walks it; 0: it could not be built (tree deeper than the
                                  traversal stack can be made, node index beyond 24 bits, scene option wide = 0) and every ray falls back to
                                  the binary rope walk — about a third of the rate                                                        */
    int32_t  wide_depth;       /* levels of the 8-wide tree (two-level scenes: TLAS levels + 1 + the deepest BLAS); the traversal kernels'
                                  LDS stack is sized from it at every launch: 320 B per wave and level                                     */
    float    wide_cost;        /* SAH cost of the 8-wide tree AS IT LIES IN MEMORY, per unit of root area: sum over child boxes (decoded as the
                                  traversal decodes them) of area x (node cost | triangle cost x triangles).  Recomputed by every build and every
                                  refit; two-level scenes: mean over the BLASes.  0 without the 8-wide layout                              */
    float    wide_cost_built;  /* the same as the last BUILD left it: wide_cost / wide_cost_built is how much refits have loosened the tree —
                                  the signal to build again (scene option "refit_max_cost_ratio" does it by itself)                         */
    uint32_t refits;           /* commits served by a refit since the last build                                                          */
    float    leaf_growth;      /* surface area of the MOVED meshes' leaf boxes against what the build gave them (1 after a build; chained over the
                                  refits since; two-level scenes: the worst BLAS).  The sharper of the two signals: a small, finely tessellated
                                  mesh in a large room hardly moves the whole tree's cost (DragonScene at a 2 % deformation: wide_cost x 1.014,
                                  leaf_growth ~2, rate x 0.85).  "refit_max_cost_ratio" acts on whichever is larger.  Both are measured on the
                                  8-wide layout: a scene built without it (wide = 0) refits its rope layout and reports 0 / 1 here       */
} MRTSceneStats;

typedef struct {
    uint64_t frames;           /* frames rendered since create/resize                          */
    uint64_t closest_rays;     /* R_closest summed over those frames                           */
    uint64_t shadow_rays;      /* R_shadow (shadow rays actually cast, Raytracing.metal:341)   */
    uint64_t primary_rays;     /* w*h (this shard's pixels) per frame, summed                  */
    uint64_t bytes_alg;        /* SURVEY §8(d) algorithmic bytes, summed                       */
    float    ms_gpu_last;      /* device ms of the last mrt_renderer_render batch (HIP events) */
    float    ms_extend_last;   /* device ms spent in the closest-hit kernel within that batch  */
    uint32_t extend_launches_last;
    uint32_t _pad;
} MRTRenderStats;

/* Device time per kernel class over the launches of the last mrt_renderer_render call that carried their own start/stop
 * events (the first 512 launches; hipExtLaunchKernelGGL events, the clock rocprofv3 --kernel-trace reads).               */
enum { MRT_KERNEL_PRIMARY = 0,   /* primary-ray generation + first closest hit                      */
       MRT_KERNEL_SHADE = 1,     /* normals, light sampling, NEE / bounce ray emission, compaction   */
       MRT_KERNEL_TRACE = 2,     /* bounce rays (closest hit) + shadow rays (any hit): the dominant kernel */
       MRT_KERNEL_ACCUMULATE = 3,
       MRT_KERNEL_CLASSES = 4 };
typedef struct {
    float    ms[MRT_KERNEL_CLASSES];          /* summed duration of the timed launches of the class   */
    uint32_t launches[MRT_KERNEL_CLASSES];    /* how many launches that sum covers                     */
} MRTKernelTimes;

typedef struct MRTContext_  *MRTContext;
typedef struct MRTScene_    *MRTScene;
typedef struct MRTRenderer_ *MRTRenderer;
typedef struct MRTGroup_         *MRTGroup;            /* n devices of one node driven by one process               */
typedef struct MRTGroupRenderer_ *MRTGroupRenderer;    /* one renderer per device of a group, image sharded by tile  */

/* ---------------------------------------------------------------- errors */
/* Message of the last failing call on this thread ("" if none).                               */
const char *mrt_last_error(void);
int         mrt_abi_version(void);

/* ---------------------------------------------------------------- context
 * replaces MTLCreateSystemDefaultDevice + makeCommandQueue (Renderer.swift:46-59).
 * Fails with MRT_ERR_NO_DEVICE when there is no HIP device — there is no CPU fallback.         */
int mrt_context_create(int device_id, MRTContext *out);
/* Handles are not reference-counted (the reference's objects are, by ARC): destroy renderers before their scene, and scenes and
 * renderers before their context.  Out of order the call is refused — MRT_ERR_STATE, nothing is freed — instead of leaving a handle
 * that points at freed memory.  NULL is accepted everywhere.                                                                    */
int mrt_context_destroy(MRTContext ctx);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int mrt_context_set_stream(MRTContext ctx, void *hip_stream);
/* The stream the context's work is enqueued on: its own, or the one mrt_context_set_stream gave it.  What a C host passes to the
 * mrt_scene_intersect_*_device entries to have a query ordered with the context's other work.                                   */
int mrt_context_get_stream(MRTContext ctx, void **hip_stream);
int mrt_context_device_name(MRTContext ctx, char *buf, size_t buflen);

/* ---------------------------------------------------------------- scene / geometry
 * replaces Model.init / Mesh.init / Submesh.init (Model.swift:13-24, Mesh.swift:18-33,
 * SubMesh.swift:23-33).  The library copies caller arrays (as MTKMeshBufferAllocator does).   */
int mrt_scene_create(MRTContext ctx, MRTScene *out);
int mrt_scene_destroy(MRTScene scene);

/* One Mesh = one instance (Renderer.swift:193-200).  positions/normals: nverts vectors with the
 * given byte stride (16 for the reference's float3 buffers, 12 for packed).  transform: 16
 * floats, column-major 4x4 object→world (Mesh.swift:21-24); the last row is ignored exactly as
 * matrix4x4_drop_last_row does (Utilities.swift:92-101).  Returns the instance id in *mesh_id.
 * Positions, normals and transforms must be finite: a NaN or an infinity is MRT_ERR_INVALID_ARGUMENT
 * here, in mrt_scene_add_instance, mrt_scene_update_mesh and mrt_scene_set_instance_transform (the
 * scene keeps what it had).                                                                     */
int mrt_scene_add_mesh(MRTScene scene, const float *positions, size_t pos_stride_bytes,
                       const float *normals, size_t nrm_stride_bytes, size_t nverts,
                       const float *transform_colmajor_4x4, int32_t *mesh_id);
/* One Submesh = one geometry of that mesh's primitive AS (Mesh.swift:39-48).  indices: 3*ntris
 * uint32 into the mesh's vertex arrays.  Returns the geometry id in *geometry_id.              */
/* A further instance of an existing mesh: shares its vertex arrays, submeshes and materials, has its own transform and its own
 * mesh id (= instance id).  The reference's counterpart is an MTLAccelerationStructureInstanceDescriptor whose
 * accelerationStructureIndex names an existing primitive structure (Renderer.swift:193-203).  With scene option instancing = 1
 * the geometry gets ONE bottom-level BVH shared by all its instances; with instancing = 0 (default) instances are flattened.   */
int mrt_scene_add_instance(MRTScene scene, int32_t source_mesh_id, const float *transform4x4_colmajor, int32_t *mesh_id);
int mrt_mesh_add_submesh(MRTScene scene, int32_t mesh_id, const uint32_t *indices, size_t ntris,
                         const MRTMaterial *material, int32_t *geometry_id);
/* Convenience = Model(name:position:rotation:scale:) (Model.swift:13): read OBJ+MTL with the
 * library's reader, build T*R*S (Mesh.swift:21-24, Utilities.swift:113-166), add mesh+submeshes. */
int mrt_scene_add_obj(MRTScene scene, const char *obj_path, const float position[3],
                      const float rotation[3], float scale, int32_t *mesh_id);
/* Scene.lights → lightBuffer (Scene.swift:15-33).                                              */
int mrt_scene_set_lights(MRTScene scene, const MRTLight *lights, int32_t count);
/* createAccelerationStructures (Renderer.swift:184-214): on-device BVH build; blocking, like the
 * reference's waitUntilCompleted (Utilities.swift:63,83).  builder: 0 = default.               */
int mrt_scene_commit(MRTScene scene);
int mrt_scene_set_option(MRTScene scene, const char *key, double value);
/* Animated transforms: replace one instance's object->world matrix (MTLAccelerationStructureInstanceDescriptor
 * .transformationMatrix, Renderer.swift:193-200); takes effect at the next mrt_scene_commit, which rebuilds the
 * world-space BVH on the device (the reference would refit/rebuild its instance AS, Renderer.swift:205-213).   */
int mrt_scene_set_instance_transform(MRTScene scene, int32_t mesh_id, const float *transform_colmajor_4x4);
/* Deforming geometry: new object-space positions and normals for the vertices of one mesh (same count, same submesh indices: the topology is kept).  The library copies
 * the arrays.  Takes effect at the next mrt_scene_commit.  When nothing else changed since the last commit, a scene with the 8-wide layout REFITS — a flattened scene its tree,
 * a two-level scene (instancing = 1) the BLAS of every changed mesh in place, in both layouts, and then its TLAS: every triangle packet rewritten, the boxes recomputed
 * bottom-up, the tree's shape as built — in a fraction of a build's time; the image is the one a fresh build of the deformed scene gives (the closest hit does not depend on
 * the tree).  The boxes of a tree that keeps its shape loosen with the deformation: MRTSceneStats.wide_cost against wide_cost_built says by how much (sah_cost follows), and
 * scene option "refit_max_cost_ratio" = r makes a commit build again by itself once wide_cost > r x wide_cost_built.  A rope layout (scene option rope = 1 beside the 8-wide one, or wide = 0 alone) is
 * refitted the same way; scene option refit = 0 builds again.  The reference builds its acceleration structures once (Renderer.swift:184-214) and never deforms a mesh; this is the counterpart of Metal's refit
 * of a primitive acceleration structure.                                                                                                                              */
int mrt_scene_update_mesh(MRTScene scene, int32_t mesh_id, const float *positions, size_t pos_stride_bytes,
                          const float *normals, size_t nrm_stride_bytes, size_t vertex_count);
int mrt_scene_stats(MRTScene scene, MRTSceneStats *out);
/* 4x3 packed instance transform as the reference stores it (Renderer.swift:193-203).          */
int mrt_scene_instance_transform(MRTScene scene, int32_t mesh_id, float out_colmajor_4x3[12]);

/* Intersector queries against the committed scene: the two uses of `intersector.intersect`
 * (Raytracing.metal:244 closest, :367 any).  Host arrays in, host arrays out.                  */
int mrt_scene_intersect_closest(MRTScene scene, const MRTRay *rays, size_t n, MRTIntersection *out);
int mrt_scene_intersect_any(MRTScene scene, const MRTRay *rays, size_t n, int32_t *occluded);
/* The same two queries on DEVICE buffers, ordered on a stream of the caller's: d_rays is n x MRTRay (32 B each), d_out n x MRTIntersection (32 B each),
 * d_occluded n x int32, all in device memory of the scene's device.  A call enqueues its kernels on hip_stream and returns: it allocates nothing, copies
 * nothing and synchronises neither the stream nor the device; the work runs after whatever that stream already holds.  A launch that fails is still
 * reported (MRT_ERR_HIP).  Every record is written; a miss is {0, -1.0f, -1, -1, -1, 0, 0, 0} as the host entries write it.
 *   hip_stream is taken literally: 0 is HIP's null stream (what torch.cuda.current_stream().cuda_stream is for torch's default stream), NOT the
 *   context's stream — a C host that wants that one asks for it with mrt_context_get_stream.
 *   The caller owes: buffers that stay alive until the stream has passed the call; no mrt_scene_commit of this scene while a query is in flight;
 *   pointers on the scene's device.
 *   Domain: finite origin and direction, 0 <= min_distance <= max_distance, max_distance may be +inf.  Inside it every field of every record has the
 *   bits mrt_scene_intersect_closest / _any return for the same ray and scene; outside it the record is unspecified, and the call still terminates.
 *   Which walk: rays with min_distance == 0 on a scene with the 8-wide layout take the render kernels' walk (lane refill, both levels of a two-level
 *   scene); the others, and every ray of a scene without that layout (scene option wide = 0), take the host entries' one-ray-per-lane walk.
 * MRT_ERR_STATE: the scene is not committed.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL buffers with n > 0, n >= 2^31.  n == 0: MRT_OK, nothing is launched. */
int mrt_scene_intersect_closest_device(MRTScene scene, const void *d_rays, size_t n, void *d_out, void *hip_stream);
int mrt_scene_intersect_any_device(MRTScene scene, const void *d_rays, size_t n, void *d_occluded, void *hip_stream);
/* ALL hits in order, on DEVICE buffers and ordered on a stream of the caller's: what lies between the first hit and the end of the ray — the surfaces a
 * shadow ray crosses, the returns of a range sensor, thickness, crossing parity.  d_rays is n x MRTRay, d_out n x max_hits x MRTIntersection (16-byte aligned),
 * d_hit_counts n x int32.  The call enqueues ONE kernel on hip_stream (taken literally, as above: 0 is HIP's null stream) and returns: it allocates nothing, copies nothing
 * and synchronises nothing; the caller owes what the two entries above ask for.
 *   A hit is a triangle whose test passes with min_distance <= t <= max_distance, both ends inclusive, as in the entries above.  Ray i's result is the max_hits SMALLEST hits
 *   under the key (distance, the library's global triangle id), ascending — the ascending id is the tie rule of the closest hit — written to d_out[i * max_hits + 0 .. count - 1]
 *   in that order; the other max_hits - count records of the row are the miss record {0, -1.0f, -1, -1, -1, 0, 0, 0}, so all max_hits records of a row are always written.
 *   d_hit_counts[i] = count, 0 .. max_hits.  Every triangle is listed at most once, also where the build split it into several references (scene option presplit).
 *   Truncation is NOT reported: once the list is full the walk prunes at its last distance and never learns whether more hits exist.  A caller who has to know asks for
 *   one more than it needs.
 *   By construction: record 0 has the bits mrt_scene_intersect_closest_device returns for the same ray; count > 0 exactly where mrt_scene_intersect_any_device says
 *   occluded; the result depends on neither the layout, the builder, nor a refit having happened.  Each record is what mrt_scene_resolve_hits_device takes: the rows
 *   reshaped to (n * max_hits) records beside each ray repeated max_hits times resolve to surfaces, the padding to miss surfaces.
 *   Domain: the closest entry's (finite origin and direction, 0 <= min_distance <= max_distance, +inf allowed); outside it the result is unspecified and the call still
 *   terminates.  One ray per lane, no lane refill (DESIGN.md §10o has the rates).
 *   Scenes: committed flattened scenes in every layout (8-wide, 8-wide + rope, wide = 0) and the empty scene (all counts 0).  A two-level scene (instancing = 1) is
 *   refused, MRT_ERR_UNSUPPORTED: the walk across both levels is not written yet.
 *   Plain arguments are checked first and a NULL scene is refused last.  MRT_ERR_INVALID_ARGUMENT: max_hits outside 1 .. MRT_MAX_HITS; n >= 2^31; n * max_hits >= 2^31;
 *   NULL buffers with n > 0; d_out not 16-byte, d_rays or d_hit_counts not 4-byte aligned; NULL scene.  MRT_ERR_STATE: the scene is not committed.  n == 0: MRT_OK, nothing
 *   is launched.  _counted (declared with its six twins below): rows at and past *d_count are touched in neither output.                                                */
#define MRT_MAX_HITS 16
int mrt_scene_intersect_all_device(MRTScene scene, const void *d_rays, size_t n, int32_t max_hits, void *d_out /* n x max_hits x MRTIntersection */,
                                   void *d_hit_counts /* n x int32 */, void *hip_stream);
/* Visibility masks: which geometry a ray may see.  Metal's intersector takes a mask with every intersect call and every instance carries one; the
 * reference declares the bits (ShaderTypes.h:23-30), sets descriptor.mask = 0xFF (Renderer.swift:196), carries a mask per submesh, and leaves its masked intersect
 * calls commented out (Raytracing.metal:243,363-365): primary rays see the light's own geometry, shadow and bounce rays do not.  The constants below are the reference's.
 *   Every mesh id — the id MRTIntersection.instance_id reports; a mesh and each instance made by mrt_scene_add_instance have their own — carries one 32-bit mask,
 *   0xFFFFFFFF until it is set.  A triangle of mesh m is VISIBLE to a ray with mask r iff (mask[m] & r) != 0; a ray mask of 0 sees nothing.
 *   mrt_scene_set_mesh_masks writes the masks of the mesh ids first_mesh_id .. + count - 1, before or after a commit.  On a committed scene it writes the device table
 *   and blocks until that is done, as a commit does (no masked query of this scene may be in flight); the tree does not depend on masks, so the call needs no commit
 *   after it and costs no build, refit or TLAS update.  Masks survive every commit and every stream-ordered update, refit and TLAS rebuild; a mesh added later has
 *   0xFFFFFFFF.  mrt_scene_get_mesh_masks reads them back.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL masks with count > 0, a range outside the scene's meshes.
 *   Draws (mrt_renderer_render) IGNORE masks: an integrator composed from the query and stage entries honours them by calling the masked entries below.          */
#define MRT_GEOMETRY_MASK_TRIANGLE 1u          /* ShaderTypes.h:23-30 */
#define MRT_GEOMETRY_MASK_LIGHT 2u
#define MRT_RAY_MASK_PRIMARY 3u
#define MRT_RAY_MASK_SHADOW 1u
#define MRT_RAY_MASK_SECONDARY 1u
int mrt_scene_set_mesh_masks(MRTScene scene, int32_t first_mesh_id, int32_t count, const uint32_t *masks);
int mrt_scene_get_mesh_masks(MRTScene scene, int32_t first_mesh_id, int32_t count, uint32_t *masks);
/* The three device queries with a visibility mask per call or per ray: ONE kernel on hip_stream (taken literally, as above), no allocation, no copy, no wait.
 *   d_ray_masks: NULL — ray_mask holds for every ray — or n x uint32 in device memory, 4-byte aligned, one per ray — ray_mask is then ignored.
 *   d_count: NULL, or one uint32 on the device with the meaning it has in the _counted entries: rows at and past it are neither read nor written.
 *   The result of ray i is, in every field and bit, what the unmasked entry of the same name returns for ray i on a scene that holds only the meshes visible to it,
 *   with the ids of the full scene: ties at equal distance go to the lowest global triangle id AMONG THE VISIBLE triangles; a triangle the ray may not see neither ends
 *   an any-hit walk, nor lowers a closest walk's bound, nor takes a slot of an all-hits list.  With every mask all-ones the entries return the unmasked entries' bits.
 *   One ray per lane, whatever min_distance is (no lane refill: DESIGN.md §10p has the rates).  In a two-level scene an instance the ray may not see is skipped before
 *   its BLAS is entered: the mask tested is the INSTANCE's, not its source mesh's.
 *   Scenes: closest and any — committed flattened scenes in every layout, two-level scenes, empty scenes; all — flattened scenes only (two-level: MRT_ERR_UNSUPPORTED,
 *   as mrt_scene_intersect_all_device).  Plain arguments are checked before the scene is looked at: MRT_ERR_INVALID_ARGUMENT for max_hits outside 1 .. MRT_MAX_HITS,
 *   n >= 2^31, n * max_hits >= 2^31, NULL buffers with n > 0, the all-hits records (its d_out) not 16-byte aligned, any other buffer not 4-byte aligned, NULL scene;
 *   MRT_ERR_STATE: the scene is not committed.  Every refusal leaves the outputs untouched.  n == 0: MRT_OK, nothing is launched.                                */
int mrt_scene_intersect_closest_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, void *d_out, void *hip_stream,
                                              const void *d_count);
int mrt_scene_intersect_any_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, void *d_occluded, void *hip_stream,
                                          const void *d_count);
int mrt_scene_intersect_all_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, int32_t max_hits, void *d_out,
                                          void *d_hit_counts, void *hip_stream, const void *d_count);
/* Deforming geometry from DEVICE buffers, ordered on a stream of the caller's: the other half of the loop "move vertices -> refit -> query or draw" on one stream.
 * mrt_scene_update_mesh_device replaces the vertices of one mesh of a COMMITTED flattened scene with vertex_count strided float3 positions and normals read from
 * device memory (strides >= 12, multiples of 4: a row of a torch view of 16 or 32 bytes is fine; 4-byte aligned pointers), in every flattened instance of that mesh;
 * mrt_scene_refit_device then refits whatever layouts are resident (the 8-wide tree, the rope layout, or both) exactly as the commit after mrt_scene_update_mesh does:
 * same kernels, same tree, same bits.  Several updates may precede one refit.  Both calls enqueue kernels on hip_stream (taken literally, as the query entries above
 * take it: 0 is HIP's null stream) and return.  The FIRST update or refit after a build creates the scene's refit workspace (about 80 B per triangle + 32 B per 8-wide
 * node; it allocates and may block) and keeps it until the next build or mrt_scene_destroy; every later call allocates nothing, copies nothing from host memory and
 * synchronises neither the stream nor the device.
 *   Validation happens on the device: a call whose positions or normals hold a NaN or an infinity writes NOTHING (the scene goes on answering with what it had, as
 *   mrt_scene_update_mesh promises) and is counted; mrt_scene_device_updates_rejected reads that count (it blocks until the calls enqueued so far have run).
 *   The caller owes: buffers that stay alive until the stream has passed the call; pointers on the scene's device; no query, draw or commit of this scene in flight on
 *   ANOTHER stream unless the caller has ordered it behind the refit (work on hip_stream itself is ordered by the stream; the renderer draws on the context's stream
 *   and on streams of its own: wait for the refit, or hand the context's stream to both, before drawing).
 *   The host side stays truthful: mrt_scene_stats (which then blocks on the last refit) reports refits, wide_cost, sah_cost, leaf_growth and build_ms as the host path
 *   would; a later mrt_scene_commit builds or refits from the vertices the device holds (it reads them back first; an update that no mrt_scene_refit_device followed
 *   counts as a vertex change, so a commit with nothing else changed refits); mrt_scene_update_mesh on such a mesh simply replaces them.  Scene option "refit_max_cost_ratio" is NOT acted on here — that would take a read-back; the statistics carry the signal and the next mrt_scene_commit may act.
 * MRT_ERR_STATE: the scene is not committed, or host-side changes wait for a commit.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL or misaligned buffers, bad strides,
 * mesh_id out of range or an instance (update its source), vertex_count other than the mesh's.  MRT_ERR_UNSUPPORTED: a two-level scene (instancing = 1: mrt_scene_update_blas_device below), scene option
 * refit = 0, or a resident tree the refit cannot take (an empty scene).                                                                                              */
int mrt_scene_update_mesh_device(MRTScene scene, int32_t mesh_id, const void *d_positions, size_t pos_stride_bytes,
                                 const void *d_normals, size_t nrm_stride_bytes, size_t vertex_count, void *hip_stream);
int mrt_scene_refit_device(MRTScene scene, void *hip_stream);
int mrt_scene_device_updates_rejected(MRTScene scene, uint64_t *count);
/* Moving the instances of a TWO-LEVEL scene (scene option instancing = 1) from DEVICE buffers, ordered on a stream of the caller's: the loop "new poses -> refit -> query
 * or draw" on one stream.  mrt_scene_set_instance_transforms_device reads `count` column-major float32 4x4 matrices (stride_bytes >= 64, a multiple of
 * 4; a 4-byte aligned pointer) for the mesh ids first_mesh_id .. first_mesh_id + count - 1, as mrt_scene_set_instance_transform takes them (the last row is forced to
 * 0 0 0 1), and rewrites in place each instance's columns, its world->object rows and its padded world box — the bits a commit computes on the host for the same matrix.
 * mrt_scene_refit_instances_device then refits the boxes of the TLAS (the rope form, and the 8-wide form when it is resident) bottom-up.  Several set calls may precede
 * one refit; a refit with nothing moved changes no answer.  Both calls enqueue kernels on hip_stream (taken literally: 0 is HIP's null stream) and return.  The FIRST of
 * them after a commit creates a small workspace (it allocates and may block) that stays until the next commit or mrt_scene_destroy; every later call allocates nothing,
 * copies nothing from host memory and synchronises neither the stream nor the device.
 *   The topology is kept: both TLAS forms keep the shape the last commit gave them, so the tree loosens as instances travel far from where it was built (the answers stay
 *   the same, the queries get slower); mrt_scene_commit builds the TLAS again from the poses the device holds.
 *   Every id must name an instance that is in the TLAS of the last commit (it has triangles and its matrix was invertible then); a commit brings the others in.
 *   Validation happens on the device: a call in which ANY matrix holds a NaN or an infinity, or has a determinant that is zero or not finite, writes NOTHING — the whole
 *   call, not the one matrix: a half-applied pose set is worse than none, and an instance cannot leave the tree without a rebuild — and is counted in the count
 *   mrt_scene_device_updates_rejected returns.
 *   The caller owes what mrt_scene_update_mesh_device asks for: live buffers on the scene's device, no use of the scene on another stream that is not ordered behind the refit.
 *   The host side stays truthful: a later mrt_scene_commit (and the replication of the scene for a device group) reads the moved instances' matrices back first, so
 *   mrt_scene_set_instance_transform on another instance + commit builds the TLAS from the poses the device holds plus the new one; mrt_scene_stats keeps working
 *   (bvh_nodes and max_depth do not change).
 * MRT_ERR_STATE: the scene is not committed, or host-side changes wait for a commit.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL or misaligned pointer, bad stride, an id
 * out of range.  MRT_ERR_UNSUPPORTED: a flattened scene (its transforms are baked into world-space triangles), a scene without an instance, an id that names an instance
 * outside the TLAS.  count == 0: MRT_OK, nothing is launched.                                                                                                          */
int mrt_scene_set_instance_transforms_device(MRTScene scene, int32_t first_mesh_id, size_t count, const void *d_transforms_colmajor_4x4, size_t stride_bytes, void *hip_stream);
int mrt_scene_refit_instances_device(MRTScene scene, void *hip_stream);
/* The TOPOLOGY of both TLAS forms of a committed two-level scene rebuilt on a stream of the caller's, from the world boxes the device holds — as
 * mrt_scene_set_instance_transforms_device and mrt_scene_refit_blas_device leave them —, followed by the refit of both forms' boxes.  It contains the
 * refit: a caller who moved poses calls EITHER mrt_scene_refit_instances_device (the tree keeps its shape and loosens as instances migrate) OR this entry (instances that
 * traded places trade leaves).  The host builders split every range of instances at half its count, so the shape of the tree depends on the instance count alone; the
 * rebuild re-sorts the instance ids under that shape by the builders' own strict order (centre sum on the widest axis, then id) and refits.  The rope form then holds the
 * nodes mrt_scene_commit would build from the same poses, bit for bit; the 8-wide form keeps the last commit's collapse (which subtrees became children of which node,
 * their slots) and gets fresh instance sets under it.  The work is enqueued on hip_stream (taken literally: 0 is HIP's null stream).  The FIRST call after a commit may
 * create or extend the instance workspace (4 bytes per instance, 12 above 1024 instances; it allocates and may block); every later call allocates nothing, copies nothing
 * from host memory and synchronises neither the stream nor the device.  Up to 1024 instances the re-sort is one launch; the limit is 65 536 instances in the TLAS.
 *   A rebuild with nothing moved changes no answer, and because the order is strict a second rebuild leaves every word of both forms as the first left it.
 *   The caller owes what mrt_scene_refit_instances_device asks for.
 *   The host side stays truthful with no new work: the next mrt_scene_commit builds both forms from the matrices it reads back; mrt_scene_stats is untouched.
 * MRT_ERR_STATE: the scene is not committed, or host-side changes wait for a commit.  MRT_ERR_UNSUPPORTED: a flattened scene, a scene with no instance in the TLAS of the
 * last commit, more than 65 536 instances in it.  MRT_ERR_INVALID_ARGUMENT: NULL scene.                                                                                  */
int mrt_scene_rebuild_tlas_device(MRTScene scene, void *hip_stream);
/* Deforming a mesh INSIDE a two-level scene (scene option instancing = 1) from DEVICE buffers, ordered on a stream of the caller's: a skinned character or
 * cloth among rigid instances, one deforming BLAS shared by many instances.  mrt_scene_update_blas_device replaces the OBJECT-space vertices of one source mesh of a
 * COMMITTED two-level scene with vertex_count strided float3 positions and normals read from device memory (strides >= 12, multiples of 4; 4-byte aligned pointers): the
 * vertices exist once, in the mesh's BLAS, and every instance of it shares them.  mrt_scene_refit_blas_device then, for every mesh updated since the last refit, refits that
 * BLAS in place in both layouts exactly as the commit after mrt_scene_update_mesh does (same kernels, same bits), gives each of its instances in the TLAS the BLAS's new
 * root box and a padded world box recomputed from it under the instance's CURRENT matrix — poses set by mrt_scene_set_instance_transforms_device are honoured, so a caller
 * who moves poses and vertices in one step needs only this refit —, and refits both TLAS forms with their topology kept.  Several updates may precede one refit; a refit
 * with nothing updated changes no answer.  Both calls enqueue kernels on hip_stream (taken literally: 0 is HIP's null stream) and return.  The FIRST of them after a commit
 * creates the BLAS workspace (the meshes' positions and indices, about 24 B per vertex and triangle, + scratch of about 100 B per triangle of the largest BLAS + 32 B per
 * 8-wide node; it allocates and may block), and the instance workspace of the entries above if it is absent; every later call allocates nothing, copies nothing from host
 * memory and synchronises neither the stream nor the device.  The workspace stays over a commit that only changes transforms and goes with every other commit.
 *   Validation happens on the device, as for mrt_scene_update_mesh_device: a call whose positions or normals hold a NaN or an infinity writes NOTHING and is counted in
 *   the count mrt_scene_device_updates_rejected returns (the sum over all the device entries of this scene).
 *   The caller owes what mrt_scene_update_mesh_device asks for: live buffers on the scene's device, no use of the scene on another stream that is not ordered behind the refit.
 *   The host side stays truthful: mrt_scene_stats (which then blocks on the last refit) reports refits, wide_cost, sah_cost, leaf_growth and build_ms as the host path would;
 *   a later mrt_scene_commit (and the replication of the scene for a device group) reads the vertices and the BLASes' root boxes back first; an update that no refit followed
 *   counts as a vertex change, so a commit with nothing else changed refits; mrt_scene_update_mesh on such a mesh simply replaces them.  Scene option
 *   "refit_max_cost_ratio" is NOT acted on here; the statistics carry the signal.
 * MRT_ERR_STATE: the scene is not committed, or host-side changes wait for a commit.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL or misaligned buffers, bad strides,
 * mesh_id out of range or an instance (update its source mesh), vertex_count other than the mesh's.  MRT_ERR_UNSUPPORTED: a flattened scene (mrt_scene_update_mesh_device
 * is for those), scene option refit = 0, a scene whose BLASes do not all have the 8-wide layout (wide = 0), a mesh whose BLAS has no 8-wide nodes or no triangles;
 * mrt_scene_refit_blas_device also for a scene with no instance in the TLAS of the last commit (as mrt_scene_refit_instances_device: nothing of it can be hit, and nothing
 * is refitted — updates made before stay pending and the next mrt_scene_commit applies them).                                                                          */
int mrt_scene_update_blas_device(MRTScene scene, int32_t mesh_id, const void *d_positions, size_t pos_stride_bytes,
                                 const void *d_normals, size_t nrm_stride_bytes, size_t vertex_count, void *hip_stream);
int mrt_scene_refit_blas_device(MRTScene scene, void *hip_stream);

/* The step after the query, on DEVICE buffers and ordered on a stream of the caller's: what the reference's kernel does right after its intersector call —
 * interpolateVertexAttribute, the instance transform of the normal and the resource-table lookup (Raytracing.metal:63-72, :261-269) — for a caller's own rays and the
 * MRTIntersection records the query entries wrote for them.  Vertex indices, normals, instance matrices and the material table live inside the library, and after
 * mrt_scene_update_mesh_device / mrt_scene_update_blas_device / mrt_scene_set_instance_transforms_device only the device holds their current values: these entries read
 * exactly those.
 *   mrt_scene_resolve_hits_device: d_rays is n x MRTRay, d_hits n x MRTIntersection, d_surfaces n x MRTSurface (64 B each); EVERY surface record is written.
 *     position   origin + direction * distance per component, a product and a sum (two roundings), the renderer's own P; `distance` is the record's
 *     normal     the renderer's shading normal: (u * n1 + v * n2) + ((1 - u) - v) * n0 of the triangle's object-space vertex normals, through columns 0..2 of
 *                the instance's matrix ((c0.k * x + c1.k * y) + c2.k * z), times 1 / sqrt of its own dot product — float32, no contraction, bit for bit what the render
 *                kernels and MRT_GUIDE_NORMAL_DEPTH hold for the same hit
 *     base_color baseColor of the material at resource_slot = instance_id * MRTSceneStats.max_submeshes + geometry_id (Renderer.swift:139), the key to the other fields
 *     A record with type == 0, and a record whose ids name nothing in the scene (instance_id, geometry_id or primitive_id negative or past the end), gives the miss record
 *     {0, 0, 0, -1.0f | 0, 0, 0, 0 | 0, 0, 0, -1 | -1, -1, -1, 0}: every id is checked against the scene's tables before anything is indexed with it.
 *   mrt_scene_interpolate_device: the general form of interpolateVertexAttribute — any per-vertex float32 data of the caller's at the hits.  d_attributes holds `channels`
 *     (1 .. 64) float32 per vertex, rows attr_stride_bytes apart (>= 4 * channels, a multiple of 4; 4-byte aligned), numbered as the caller knows the vertices: the source
 *     meshes concatenated in mesh-id order, an instance sharing its source's rows (mrt_scene_vertex_offsets: each mesh's first row — an instance reports its source's — and,
 *     last, the total).  For a hit on the triangle (i0, i1, i2): out[c] = (u * a[i1][c] + v * a[i2][c]) + ((1.0f - u) - v) * a[i0][c], float32, no contraction; a miss or
 *     an invalid id writes 0 in every channel.  d_out: n rows of `channels` float32, out_stride_bytes apart (same rules); bytes between the rows are left alone.
 * Both scene forms and every layout (8-wide, 8-wide + rope, rope only): the tree is not read.
 * The contract of the _device query entries: buffers in device memory of the scene's device that stay alive until the stream has passed the call; hip_stream taken literally
 * (0 is HIP's null stream); no mrt_scene_commit while a call is in flight, and device updates of the scene on ANOTHER stream ordered by the caller.  The FIRST call after a
 * commit creates a table of 16 bytes per resource slot (it allocates and may block); every later call enqueues one kernel and returns: it allocates nothing, copies nothing
 * from host memory and synchronises neither the stream nor the device.  Nothing here writes the scene, so the stale-host rules of mrt_scene_update_mesh_device do not apply.
 * n == 0: MRT_OK, nothing is launched.  MRT_ERR_STATE: the scene is not committed.  MRT_ERR_INVALID_ARGUMENT: NULL scene, NULL buffers with n > 0, d_rays / d_hits /
 * d_surfaces not 16-byte aligned, attributes / output not 4-byte aligned, channels outside 1 .. 64, a bad stride, n >= 2^31; mrt_scene_vertex_offsets: count other than
 * the number of meshes + 1.                                                                                                                                             */
typedef struct {
    float   position[3];   float   distance;       /* origin + direction * distance | the record's distance (-1 for a miss)                   */
    float   normal[3];     int32_t type;           /* shading normal, world space, normalised | 1 = triangle, 0 = none                        */
    float   base_color[3]; int32_t resource_slot;  /* base_color[instance * max_submeshes + geometry] | that slot (-1 for a miss)             */
    int32_t instance_id, geometry_id, primitive_id, _pad;
} MRTSurface;                                                         /* 64 B                   */
int mrt_scene_resolve_hits_device(MRTScene scene, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, void *hip_stream);
int mrt_scene_interpolate_device(MRTScene scene, const void *d_hits, size_t n, const void *d_attributes, size_t attr_stride_bytes, int32_t channels,
                                 void *d_out, size_t out_stride_bytes, void *hip_stream);
int mrt_scene_vertex_offsets(MRTScene scene, uint64_t *offsets /* meshes + 1 entries */, size_t count);

/* The two steps of the reference's kernel that frame the query and the surface lookup, on DEVICE buffers and ordered on a stream of the caller's: where the
 * rays come from (Raytracing.metal:171-221) and what follows a surface (:272-391) — the light pick and its evaluation, the next-event shadow ray, the cosine-hemisphere
 * bounce.  With them the reference's integrator, or a variant of it, is five stream-ordered calls — generate, mrt_scene_intersect_closest_device,
 * mrt_scene_resolve_hits_device, scatter, mrt_scene_intersect_any_device — and element-wise arithmetic of the caller's (throughput = throughput * base_color; radiance +=
 * light * throughput where the shadow ray got through); composed so, the image is the renderer's own, bit for bit.  Materials extension OFF: these are the expressions of
 * the reference's diffuse path; the semantics of renderer option materials = 1 are mrt_scene_scatter_materials_device's, below.
 *   mrt_renderer_primary_rays_device: for every pixel p = y * width + x of the renderer's image (row 0 at the bottom, as mrt_renderer_read_accum; the WHOLE image whatever
 *     the renderer's shard) d_halton_index[p] = (int32)(hash(seed, p) + sample_index), the renderer's own per-pixel seed plus the caller's sample index with wrap-around,
 *     and d_rays[p] = {camera position | 0, normalize((uvx * right + uvy * up) + forward) | +inf} with uv = ((x, y) + halton(index, 0 and 1)) / (width, height) * 2 - 1:
 *     the primary ray mrt_renderer_render traces for that pixel at Uniforms.frameIndex == sample_index (renderer option sample_offset is not added: pass it in).  Reads the
 *     camera as mrt_renderer_set_camera left it and the renderer's width and height; writes nothing of the renderer's and does not advance the frame index.
 *   mrt_scene_scatter_device: row i in, row i out, no compaction.  d_surfaces is n x MRTSurface as mrt_scene_resolve_hits_device wrote them (position, normal and type are
 *     read), d_halton_index n x int32 as above, `bounce` the path depth of these surfaces (0 for primary hits; at most 18: five Halton dimensions per bounce from dimension
 *     2 on, and the prime table holds 100), light_count Uniforms.lightCount (0 = every light of the scene; more than the scene holds is refused).  For a surface with
 *     type == 1:
 *       the light    li = min((int)(halton(index, 2 + 5 * bounce) * light_count), light_count - 1); its direction, distance and colour by the light's type (an area light
 *                    takes dimensions + 1 and + 2), * saturate(dot(normal, direction)) * light_count               -> d_light[i] = {colour | wanted ? 1.0f : 0.0f}
 *       wanted       length(colour) > 0.0001f: the reference traces a shadow ray only then
 *       shadow ray   {position + normal * 1e-3f | 0, direction to the light | its distance - 1e-3f (+inf for a sun)}  -> d_shadow_rays[i], when wanted
 *       bounce ray   {position + normal * 1e-3f | 0, the cosine-weighted direction about the normal from dimensions + 3 and + 4 | +inf}      -> d_next_rays[i]
 *     A row whose type is not 1 gives zeros in all three outputs, and a shadow ray that is not wanted is 32 zero bytes (the light row then still holds the colour that
 *     fell below the threshold, with 0 in its fourth component).  A zero ray — zero direction, max_distance 0 — is inside the query entries' domain, but what they answer
 *     for it is unspecified: go by the light row's fourth component and by the surface's type, never by the answer to such a row.  d_light is n x 4 float32;
 *     d_next_rays may be NULL (the last bounce): nothing is computed for it.  The entry reads the scene's light table only — no tree and no geometry — so both scene forms
 *     and every layout take one path.
 * float32, no contraction, IEEE divide and square root: the bits the render kernels hold for the same pixel.  The contract of the _device query entries: buffers in device
 * memory of the renderer's / scene's device, alive until the stream has passed the call; hip_stream taken literally (0 is HIP's null stream); each call enqueues one kernel
 * and returns — no allocation, no copy from host memory, no wait; no mrt_scene_set_lights or mrt_scene_commit while a call is in flight.
 * Plain arguments are checked first and a NULL handle last.  MRT_ERR_INVALID_ARGUMENT: NULL buffers (scatter: with n > 0), rays / surfaces / light rows not 16-byte
 * aligned, the index not 4-byte aligned, n >= 2^31, bounce < 0 or > 18, light_count < 0 or above the scene's, a NULL handle.  MRT_ERR_STATE: the scene is not committed or
 * has no light (as mrt_renderer_render).  n == 0: MRT_OK, nothing is launched.                                                                                          */
int mrt_renderer_primary_rays_device(MRTRenderer r, uint32_t sample_index, void *d_rays /* w*h x MRTRay */, void *d_halton_index /* w*h x int32 */, void *hip_stream);
int mrt_scene_scatter_device(MRTScene scene, const void *d_surfaces /* n x MRTSurface */, const void *d_halton_index /* n x int32 */, size_t n, int32_t bounce, int32_t light_count,
                             void *d_shadow_rays /* n x MRTRay */, void *d_light /* n x 4 float32 */, void *d_next_rays /* n x MRTRay, may be NULL */, void *hip_stream);

/* mrt_scene_scatter_device with the materials extension ON: what follows a surface when renderer option materials = 1 — emission, the lobe choice, the
 * dielectric interface, the GGX specular lobe, and the diffuse path above with its albedo divided by the probability of having been chosen.  Row i in, row i out, no
 * compaction.  d_rays is n x MRTRay, the rays that hit these surfaces (the direction is read); d_surfaces, d_halton_index, light_count as above; max_bounces is the
 * renderer's option (1 .. 16) and 0 <= bounce < max_bounces: the lobe choice reads Halton dimension 2 + 5 * max_bounces + bounce, which stays below the prime table's 100.
 * For a surface with type == 1 whose resource_slot lies in [0, instances * max_submeshes) the material is the scene's at that slot, with ONE exception: the albedo is the
 * row's base_color (an unmodified row holds the material's; a caller may substitute their own), for kd = max(base_color) and for the diffuse weight alike.  With
 * ks = max(specular), trn = 1 - dissolve where 0 < dissolve < 1 and refractionIndex > 0 (else 0), u = halton(index, 2 + 5 * max_bounces + bounce):
 *   u < trn                the dielectric interface: Schlick's Fresnel term at u / trn picks reflection (lobe 2) or refraction (lobe 3; total internal reflection is lobe 2);
 *                          weight {1, 1, 1}; continuation {position + nn * 1e-3f (reflected) or * -1e-3f (refracted) | 0, normalize(nd) | +inf}, nn the normal facing the ray
 *   else, with ud = (u - trn) / (1 - trn) where trn > 0 (else u) and ps = ks / (ks + kd) where ks > 0 and specularExponent > 0 (else 0):
 *   ud < ps                the specular lobe: the ray mirrored about a GGX half vector (alpha^2 = 2 / (Ns + 2)) from dimensions 2 + 5 * bounce + 3 and + 4.  Above the
 *                          surface: lobe 4, weight specular * (1 / ps), continuation {position + normal * 1e-3f | 0, normalize(wi) | +inf}.  Below it: lobe 5, the
 *                          path is absorbed — weight {0, 0, 0}, no continuation
 *   else                   the diffuse path: lobe 1, weight base_color (* (1 / (1 - ps)) where ps > 0); d_shadow_rays[i], d_light[i] and the cosine-weighted
 *                          d_next_rays[i] exactly as mrt_scene_scatter_device writes them
 * d_lobes[i] = {weight | lobe, the material's emission | 0} (MRTScatterLobe).  The dielectric and specular lobes make no next-event estimate: their d_shadow_rays and
 * d_light rows are zeros.  A row that is no surface — type != 1, or a resource_slot outside the scene's table (nothing is indexed with it) — gives zeros in all four
 * outputs (lobe 0); an absorbed row gives zeros but its lobe code and emission.  d_next_rays may be NULL: every other output keeps its bits.  A frame of the
 * renderer's integrator is then, per bounce and in this order: radiance += throughput * emission; throughput *= weight; radiance += light.rgb * throughput where
 * light.w == 1 and the shadow ray got through; the path goes on where lobe is 1, 2, 3 or 4 — composed so, the image is mrt_renderer_render's with materials = 1, bit
 * for bit.  One kernel per call; the contract, the refusal rules and their order are mrt_scene_scatter_device's, with d_rays and d_lobes 16-byte aligned and required,
 * max_bounces outside 1 .. 16 and bounce outside [0, max_bounces) refused.                                                                                               */
typedef struct {
    float   weight[3];     int32_t lobe;           /* factor of the throughput | 0 none, 1 diffuse, 2 interface reflected, 3 interface refracted, 4 specular, 5 absorbed */
    float   emission[3];   int32_t _pad;           /* the material's emission, not multiplied by any throughput | 0                                                   */
} MRTScatterLobe;                                                     /* 32 B                   */
int mrt_scene_scatter_materials_device(MRTScene scene, const void *d_rays /* n x MRTRay */, const void *d_surfaces /* n x MRTSurface */, const void *d_halton_index /* n x int32 */, size_t n,
                                       int32_t bounce, int32_t max_bounces, int32_t light_count, void *d_shadow_rays /* n x MRTRay */, void *d_light /* n x 4 float32 */,
                                       void *d_next_rays /* n x MRTRay, may be NULL */, void *d_lobes /* n x MRTScatterLobe */, void *hip_stream);

/* Row queues on DEVICE buffers, ordered on a stream of the caller's: what a wavefront integrator needs between two of the stage entries above — the rows
 * that go on (the surviving paths, the wanted shadow rays) moved to the front of their buffers, and their number left in a word ON THE DEVICE that the next stage reads.
 *   mrt_context_compact_rows_device: with m = min(n, *d_count_in) (n when d_count_in is NULL) and k_0 < k_1 < ... the rows i < m whose byte d_keep[i] is not 0,
 *     *d_count_out is their number and, for each of the `ncolumns` (0 .. 8) columns, dst row j is src row k_j, byte for byte: the ORDER IS KEPT (what x[:m][mask[:m]] gives),
 *     so a frame composed from queues is the same from run to run.  A column is {src, dst, row_bytes}: row_bytes a multiple of 4 in 4 .. 64; src and dst 16-byte aligned
 *     where row_bytes is a multiple of 16 (the rows then move as 16-byte vectors), 4-byte aligned otherwise (dwords).  dst rows from *d_count_out on are neither read nor
 *     written; src, d_keep and d_count_in are only read.  ncolumns == 0 is a count alone.  `columns` is a HOST array, read during the call; the pointers in it, d_keep
 *     (n x uint8; a torch.bool tensor is one), d_count_in, d_count_out (one uint32 each, 4-byte aligned) and d_workspace are device pointers.  The count word is read as
 *     unsigned: one above n, or negative, is clamped to n.
 *     d_workspace is the call's scratch memory: at least mrt_compact_workspace_bytes(n) bytes (4 bytes per 2048 rows, rounded up to 16; never 0; it does not decrease with
 *     n), 16-byte aligned, the caller's — nothing hides inside the handle, so two streams may compact at once, each with a workspace of its own.
 *     Three kernels on hip_stream — count per workgroup, one scan of the totals, the move — and nothing else: no allocation, no copy from host memory, no wait, no atomics,
 *     and no workgroup ever waits for another.  hip_stream is taken literally (0 is HIP's null stream).  The caller owes buffers on the context's device that stay alive until
 *     the stream has passed the call.
 *     Plain arguments are checked first, the message names the argument, and a NULL context is refused last.  MRT_ERR_INVALID_ARGUMENT: n >= 2^31; NULL d_keep, d_count_out
 *     or d_workspace with n > 0; d_count_in or d_count_out not 4-byte aligned; d_count_out == d_count_in; ncolumns outside 0 .. 8, NULL columns with ncolumns > 0; a
 *     row_bytes that is 0, above 64 or no multiple of 4; a misaligned or NULL src or dst; a dst range [dst, dst + n * row_bytes) that overlaps its own src range, another
 *     column's dst range, d_keep or either count word; a workspace that is misaligned or too small.  n == 0: 0 is written to *d_count_out (where it is given), MRT_OK.
 *   The *_device_counted entries are their twins above with one more argument, d_count: one uint32 on the device, 4-byte aligned, REQUIRED (the twin is the form without
 *     it).  n is then the CAPACITY of the buffers: the kernels handle the rows i < min(n, *d_count) — the word is read as unsigned, once, when a kernel starts; too large or
 *     negative is clamped to n — and give for them exactly what the twin writes for them; no row from there on is read or written.  Everything else is the twin's:
 *     arguments, refusal rules and their order (d_count is looked at first), first-call behaviour, which walk a ray takes.  Grids are sized by n: a workgroup past the
 *     count leaves at once, so a call costs its launch however short the queue.                                                                                          */
typedef struct { const void *src; void *dst; uint32_t row_bytes; uint32_t _pad; } MRTRowColumn;   /* 24 B */
size_t mrt_compact_workspace_bytes(size_t n);
int mrt_context_compact_rows_device(MRTContext ctx, const void *d_keep /* n x uint8, non-zero keeps */, size_t n, const void *d_count_in /* 1 x uint32, may be NULL */,
                                    const MRTRowColumn *columns, int32_t ncolumns /* 0 .. 8 */, void *d_count_out /* 1 x uint32 */, void *d_workspace, size_t workspace_bytes,
                                    void *hip_stream);
int mrt_scene_intersect_closest_device_counted(MRTScene scene, const void *d_rays, size_t n, void *d_out, void *hip_stream, const void *d_count);
int mrt_scene_intersect_any_device_counted(MRTScene scene, const void *d_rays, size_t n, void *d_occluded, void *hip_stream, const void *d_count);
int mrt_scene_intersect_all_device_counted(MRTScene scene, const void *d_rays, size_t n, int32_t max_hits, void *d_out, void *d_hit_counts, void *hip_stream, const void *d_count);
int mrt_scene_resolve_hits_device_counted(MRTScene scene, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, void *hip_stream, const void *d_count);
int mrt_scene_interpolate_device_counted(MRTScene scene, const void *d_hits, size_t n, const void *d_attributes, size_t attr_stride_bytes, int32_t channels,
                                         void *d_out, size_t out_stride_bytes, void *hip_stream, const void *d_count);
int mrt_scene_scatter_device_counted(MRTScene scene, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t light_count,
                                     void *d_shadow_rays, void *d_light, void *d_next_rays /* may be NULL */, void *hip_stream, const void *d_count);
int mrt_scene_scatter_materials_device_counted(MRTScene scene, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t max_bounces,
                                               int32_t light_count, void *d_shadow_rays, void *d_light, void *d_next_rays /* may be NULL */, void *d_lobes, void *hip_stream,
                                               const void *d_count);

/* The integrator's path state on DEVICE buffers, ordered on a stream of the caller's: what lies between the stage entries above — throughput x colour,
 * emission along the path, the keep masks the two compactions of a bounce take, radiance += light x throughput where the shadow ray got through, the running average.
 * With them a frame on queues is library calls only, with no host read and no element-wise pass of the caller's.  None of the four reads a scene.
 *   Common: each call enqueues ONE kernel on hip_stream (taken literally; 0 is HIP's null stream) and nothing else: no allocation, no copy from host memory, no wait.
 *     Buffers are on the context's device and stay alive until the stream has passed the call.  Ray, throughput, light, radiance, MRTSurface and MRTScatterLobe rows are
 *     16-byte aligned; index, count and occluded words 4-byte aligned.  d_count is one uint32 on the device and may be NULL: the kernels handle the rows i < m,
 *     m = min(n, *d_count) (n when NULL); the word is read as unsigned, once, when the kernel starts, and no row from m on is read or written.  n == 0 is MRT_OK and
 *     launches nothing.  d_radiance is npixels rows of 4 float32; only .rgb is ever changed.  A pixel word is read as unsigned and a row whose pixel is >= npixels
 *     deposits nothing: nothing outside the image is touched, whatever a row holds.  The caller owes that a pixel occurs AT MOST ONCE among the rows < m of one call
 *     (true of every queue the compaction above makes of distinct pixels): the deposit is a plain load, add and store, no atomics, and the image is the same from run to
 *     run; where the caller breaks this, that pixel's sum is unspecified and nothing else is.  Arithmetic is float32, one rounding per * and per +, IEEE divide.
 *     Plain arguments are checked first, the message names the argument, and a NULL context is refused last.  MRT_ERR_INVALID_ARGUMENT: n or npixels >= 2^31, a
 *     required buffer that is NULL with n > 0, a misaligned buffer, and what each entry adds below.
 *   mrt_context_reset_paths_device: the state before bounce 0 — throughput[i] = {1, 1, 1, 1} and pixel[i] = i for i < n, radiance[p] = {0, 0, 0, 0} for p < npixels where
 *     d_radiance is given.
 *   mrt_context_advance_paths_device: the step after scatter.  EXACTLY ONE of d_surfaces / d_lobes is given (both, or neither, is refused).
 *     Diffuse form (d_surfaces, the rows of mrt_scene_resolve_hits_device; only their normal | type and base_color | slot groups are read): on = type == 1;
 *     thr.rgb = thr.rgb * base_color for every row < m; keep_path = on; keep_shadow = on && light.w == 1.0f.  d_pixel and d_radiance are not read and may be NULL.
 *     Materials form (d_lobes, the rows of mrt_scene_scatter_materials_device; d_pixel and d_radiance are required): where lobe != 0,
 *     radiance[pixel].rgb = radiance[pixel].rgb + thr.rgb * emission with the throughput BEFORE its update; then thr.rgb = thr.rgb * weight for every row < m;
 *     keep_path = 1 <= lobe <= 4; keep_shadow = light.w == 1.0f.
 *     thr.w keeps its bits.  The mask bytes are written as 0 or 1 for every row < m; d_keep_path may be NULL (the last bounce: no second mask is written).
 *   mrt_context_deposit_light_device: the step after the any-hit query on the compacted shadow queue — for the rows < m with occluded == 0,
 *     radiance[pixel].rgb = radiance[pixel].rgb + light.rgb * thr.rgb.
 *   mrt_context_fold_sample_device: the reference's running average of a frame's sample into the accumulation — frame_index == 0: accum.rgb = sample.rgb; otherwise
 *     accum.rgb = (sample.rgb + accum.rgb * (float)frame_index) / (float)(frame_index + 1); accum.w = 1.0f, as the renderer writes it.  clear_sample != 0 leaves the sample
 *     rows as zeros for the next frame, in the same pass.  frame_index == 2^32 - 1 and d_sample == d_accum are refused.  d_accum goes straight into
 *     mrt_renderer_write_accum_from_device: the tonemap and the denoiser then apply to a composed image.                                                                 */
int mrt_context_reset_paths_device(MRTContext ctx, size_t n, void *d_throughput /* n x 4 float32 */, void *d_pixel /* n x uint32 */, void *d_radiance /* may be NULL */,
                                   size_t npixels, void *hip_stream);
int mrt_context_advance_paths_device(MRTContext ctx, size_t n, const void *d_count /* may be NULL */, const void *d_surfaces /* n x MRTSurface or NULL */,
                                     const void *d_lobes /* n x MRTScatterLobe or NULL */, const void *d_light /* n x 4 float32 */, void *d_throughput /* in and out */,
                                     const void *d_pixel, void *d_radiance, size_t npixels, void *d_keep_shadow /* n x uint8 */, void *d_keep_path /* n x uint8, may be NULL */,
                                     void *hip_stream);
int mrt_context_deposit_light_device(MRTContext ctx, size_t n, const void *d_count /* may be NULL */, const void *d_occluded /* n x int32 */, const void *d_light,
                                     const void *d_throughput, const void *d_pixel, void *d_radiance, size_t npixels, void *hip_stream);
int mrt_context_fold_sample_device(MRTContext ctx, size_t npixels, void *d_sample, void *d_accum, uint32_t frame_index, int32_t clear_sample, void *hip_stream);

/* ---------------------------------------------------------------- host-side geometry helpers
 * (no GPU needed) — the library's OBJ/MTL reader standing in for ModelIO (Model.swift:16-21,
 * SubMesh.swift:37-54) and the procedural dragon proxy (dragon.obj is absent upstream).        */
typedef struct MRTMeshData_ *MRTMeshData;
int mrt_obj_load(const char *obj_path, MRTMeshData *out);
int mrt_dragon_proxy(MRTMeshData *out);             /* exactly 871 414 triangles               */
int mrt_dragon_proxy_irregular(MRTMeshData *out);   /* same count / extents / material, irregular connectivity, shuffled order (sensitivity check) */
int mrt_dragon_proxy_hostile(MRTMeshData *out);     /* same count / extents / material; triangle sizes over 100 : 1 and 1 % slivers of up to 50 x their edge (stress test of the builder) */
int mrt_bunny_proxy(MRTMeshData *out);              /* exactly  69 451 triangles               */
int mrt_meshdata_free(MRTMeshData m);
int mrt_meshdata_counts(MRTMeshData m, size_t *nverts, int32_t *nsubmeshes);
/* positions / normals: nverts*3 packed floats */
int mrt_meshdata_vertices(MRTMeshData m, float *positions, float *normals);
int mrt_meshdata_submesh(MRTMeshData m, int32_t submesh, size_t *ntris, uint32_t *indices /* may be NULL */,
                         MRTMaterial *material /* may be NULL */, char *name_buf, size_t name_buflen);
/* T*R*S with R = Rx*Ry*Rz (Mesh.swift:21-24; Utilities.swift:104-166), column-major 4x4.       */
int mrt_make_transform(const float position[3], const float rotation[3], float scale, float out16[16]);
/* Scene.setupCamera(size:) (Scene.swift:40-57).                                                */
int mrt_default_camera(int32_t width, int32_t height, MRTCamera *out);

/* ---------------------------------------------------------------- renderer
 * replaces Renderer.init / createTextures / createBuffers (Renderer.swift:45-71, :107-182,
 * :231-275).  seed drives the per-pixel Halton offsets (the reference uses arc4random, :259).
 * max_bounces: the literal 3 of Raytracing.metal:237.                                         */
int mrt_renderer_create(MRTContext ctx, MRTScene scene, int32_t width, int32_t height,
                        uint32_t seed, int32_t max_bounces, MRTRenderer *out);
int mrt_renderer_destroy(MRTRenderer r);
/* mtkView(_:drawableSizeWillChange:) (Renderer.swift:353-356): new targets, new seeds, frameIndex=0 */
int mrt_renderer_resize(MRTRenderer r, int32_t width, int32_t height);
/* Default camera = Scene.setupCamera(size) recomputed from the size (Scene.swift:36-57).       */
int mrt_renderer_set_camera(MRTRenderer r, const MRTCamera *camera);
/* updateUniforms (Renderer.swift:216-229) in one call: the 96-byte Uniforms block the reference binds at buffer index 0
 * (ShaderTypes.h:89-97, Renderer.swift:304).  A new width / height resizes (new targets and seeds, Renderer.swift:353-356, and
 * the given frameIndex is applied after that); frameIndex is the accumulation weight and Halton index of the next frame;
 * lightCount in [1, lights of the scene] makes the kernels sample only the first lightCount lights (Raytracing.metal:273, :335);
 * blocksWide is ignored (derived from the size; the reference's kernel never reads it).  get_uniforms returns what the next
 * frame will be drawn with.                                                                                                 */
int mrt_renderer_set_uniforms(MRTRenderer r, const MRTUniforms *uniforms);
int mrt_renderer_get_uniforms(MRTRenderer r, MRTUniforms *uniforms);
/* The renderer's knobs.  The reference's own: "max_bounces" (the literal 3 of Raytracing.metal:237; 1..19), "frames_in_flight"
 * (Renderer.maxFramesInFlight, Renderer.swift:33: here passes in flight on separate HIP streams, default 3 as the reference), "sample_offset" (added to
 * frameIndex for the Halton index only: sample-index sharding).  This implementation's: "frame_batch" (frames carried through the pipeline
 * per pass, 1..32: larger launches against more queue memory — "lane_bytes" per pass in flight; 0, the default, sizes it by the image: 8 at 1920 x 1080 pixels
 * per device and above, proportionally more for a smaller image or a shard of one, so that a pass always carries about the same number of pixel-frames; reads back as the value in force), "megakernel" (1: one launch
 * per frame, the lowest latency of a single frame; the default pipeline has the higher throughput), "materials" (1: the materials
 * extension — emission, specular lobe, refraction; max_bounces <= 16; the only key that changes the image), "guides" (1: the first-hit guide buffers the denoiser reads, see mrt_renderer_read_guide below).  Read-only through
 * mrt_renderer_get_option: "lanes_used", "lane_bytes".                                                                              */
int mrt_renderer_set_option(MRTRenderer r, const char *key, double value);
int mrt_renderer_get_option(MRTRenderer r, const char *key, double *value);
/* Screen-tile shard for multi-GPU: this renderer owns 8x8 tiles with (tile_id % world) == rank;
 * other pixels stay 0 in its targets so that a sum-reduce assembles the frame.                 */
int mrt_renderer_set_shard(MRTRenderer r, int32_t rank, int32_t world);
/* Restart accumulation at a given frame index (sample-index sharding; resume).                 */
int mrt_renderer_set_frame_index(MRTRenderer r, uint32_t frame_index);
int mrt_renderer_frame_index(MRTRenderer r, uint32_t *frame_index);
/* draw(in:) (Renderer.swift:284-351) n_frames times: enqueue on the stream and return.         */
int mrt_renderer_render(MRTRenderer r, int32_t n_frames);
/* commandBuffer completion (Renderer.swift:285-287).                                           */
int mrt_renderer_wait(MRTRenderer r);
/* The same completion as a poll (the reference's handler is told per command buffer, Renderer.swift:285-287): frames, counted
 * as MRTRenderStats.frames is, whose accumulation has finished on the device.  Never blocks.  Granularity: a pass of `frame_batch`
 * frames; the LAST passes of a draw call (one per pass in flight, i.e. every pass of a short call such as 20 frames) are accumulated
 * together when the call's last traversal launch has finished, so their frames are reported together at the end of the call.  A call
 * whose passes carry ONE frame each runs every pass as groups of tiles on several streams and reports its frames at the end of the call.  */
int mrt_renderer_frames_completed(MRTRenderer r, uint64_t *frames);
/* accumulationTargets[0] after the swap (Renderer.swift:332-334): w*h RGBA32F, row 0 = bottom of
 * the image as the kernel writes it (Raytracing.metal:206-207; the blit flips, Shaders.metal:35). */
int mrt_renderer_read_accum(MRTRenderer r, float *rgba, size_t nbytes);
/* Same data copied device→device into caller memory (e.g. a torch tensor for the RCCL reduce). */
int mrt_renderer_copy_accum_to_device(MRTRenderer r, void *device_ptr, size_t nbytes);
int mrt_renderer_write_accum_from_device(MRTRenderer r, const void *device_ptr, size_t nbytes);
/* The compact assemble of a tile-sharded image (beside the reduce(sum) of whole buffers that BASELINE.json's north_star prescribes and mrt_group_gather defaults to): a rank
 * ships only the pixels it owns — 1 / world of the image — and the root writes them in place.  A compact buffer is tiles x 64 RGBA32F pixels, device memory: tile lt of shard
 * (rank, world) is tile lt * world + rank of the image (8 x 8 tiles, row-major over the image), its pixels row-major, pixels outside the image 0.
 *   _shard_tiles   tiles of this renderer's image that shard (rank, world) owns
 *   _pack_owned    this renderer's accumulation buffer -> the compact buffer of ITS shard (mrt_renderer_set_shard), enqueued on its stream
 *   _unpack_tiles  the compact buffer of shard (rank, world) -> this renderer's accumulation buffer, at those tiles' pixels
 *   _unpack_tiles_into  the same into `image` instead (device memory, width*height*16 bytes of this renderer's size), enqueued on its stream: the root assembles the
 *                  image in a buffer of its own and its accumulation buffer keeps its shard (a later draw or reduce would otherwise carry the other shards' pixels)  */
int mrt_renderer_shard_tiles(MRTRenderer r, int32_t rank, int32_t world, uint64_t *tiles);
int mrt_renderer_pack_owned_tiles(MRTRenderer r, void *device_ptr, size_t nbytes);
int mrt_renderer_unpack_tiles(MRTRenderer r, const void *device_ptr, size_t nbytes, int32_t rank, int32_t world);
int mrt_renderer_unpack_tiles_into(MRTRenderer r, void *image, size_t image_nbytes, const void *device_ptr, size_t nbytes, int32_t rank, int32_t world);
/* fragmentShader (Shaders.metal:39-52): Reinhard c/(1+c), top row first (flipped), RGBA8.      */
int mrt_renderer_read_tonemapped_rgba8(MRTRenderer r, uint8_t *rgba, size_t nbytes);
int mrt_renderer_stats(MRTRenderer r, MRTRenderStats *out);
int mrt_renderer_reset_stats(MRTRenderer r);
int mrt_renderer_kernel_times(MRTRenderer r, MRTKernelTimes *out);   /* waits for the last render call */

/* ---------------------------------------------------------------- first-hit guide buffers and the denoiser
 * NOT in the reference: its only outputs are the accumulation target and the tonemap into the drawable (Renderer.swift:284-351); like the
 * materials extension this is defined here.  With renderer option "guides" = 1 every mrt_renderer_render call also maintains three per-pixel
 * buffers of the PRIMARY hit, laid out like the accumulation buffer (width*height entries of 16 bytes, row 0 = bottom of the image):
 *   MRT_GUIDE_NORMAL_DEPTH  4 x float32  xyz: shading normal of the hit (normalised, world space), w: hit distance t
 *   MRT_GUIDE_ALBEDO        4 x float32  rgb: baseColor of the hit submesh's material, a: 1 (coverage)
 *   MRT_GUIDE_IDS           4 x int32    {type, instance_id, geometry_id, primitive_id} as MRTIntersection names them; a miss is {0, -1, -1, -1}
 * A frame whose primary ray misses contributes zeros to the first two, which are running averages over the frames with the accumulation
 * buffer's own rule and weights (Raytracing.metal:395-401: frameIndex == 0 replaces, otherwise (new + old * frameIndex) / (frameIndex + 1)), so
 * the coverage is the share of frames that hit; the ids are those of the most recent frame.  The primary ray of a frame is the one its colour
 * path starts with.  Resize and set_shard clear the guides; pixels a shard does not own stay all-zero.  The guides are complete when
 * mrt_renderer_wait returns; they cost one more walk of the primary rays per frame, in a kernel of their own, and with "guides" = 0 (default)
 * nothing is allocated or launched.  Set the option BEFORE frame 0 (or call mrt_renderer_set_frame_index(r, 0) after setting it): switched on at
 * frame f > 0 the averages start from zero buffers with weight f / (f + 1), so normals, distance and coverage are scaled by about 1 / (f + 1) and
 * the denoiser's normal term rejects every tap — the image comes back unfiltered.  MRT_ERR_STATE with "guides" = 0 or before a frame was rendered with it on.                           */
enum { MRT_GUIDE_NORMAL_DEPTH = 0, MRT_GUIDE_ALBEDO = 1, MRT_GUIDE_IDS = 2, MRT_GUIDE_COUNT = 3 };
int mrt_renderer_read_guide(MRTRenderer r, int32_t which, void *out, size_t nbytes);
int mrt_renderer_copy_guide_to_device(MRTRenderer r, int32_t which, void *device_ptr, size_t nbytes);
/* Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) of the accumulation buffer, guided by the normal / depth and
 * albedo buffers, into a separate RGBA32F "denoised" buffer; the accumulation buffer is not modified.  Enqueued on the renderer's stream after
 * everything rendered so far.  float32 throughout, operations in the order written:
 *   A_p = max(albedo_p.rgb, 1e-3) per channel if demodulate and the pixel's coverage is not 0, else 1;  I_p = accum_p.rgb / A_p.  A pixel with
 *   coverage 0 (no frame hit anything) is copied through in every iteration — its output is its accumulation value bit for bit — and is never a
 *   tap of another pixel.  Iteration i (step = 1 << i, sc = sigma_color / step): over the 25 taps q = p + step * (dx, dy),
 *   dy outer, dx inner, both -2 .. 2, skipping taps outside the image or of coverage 0; B = {1/16, 1/4, 3/8, 1/4, 1/16}, k(x) = max(0, 1 - x),
 *   lum(c) = (0.2126 r + 0.7152 g) + 0.0722 b:
 *     h = B[dy + 2] * B[dx + 2];  xn = (1 - max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)) / sigma_normal;
 *     xz = |t_p - t_q| / ((sigma_depth * t_p) * step);  xc = |lum(I_p) - lum(I_q)| / sc;
 *     w = ((h * k(xn)^2) * k(xz)^2) * k(xc)^2 — the centre tap takes w = h;  sum += w * I_q, wsum += w;  I'_p = sum / wsum.
 *   Output rgb = I_last * A_p, alpha 1.  n and t are the averaged guide values as stored.  A covered pixel all of whose taps have weight 0 comes
 *   back as (h I_p) / h with h = 9/64: its value to two roundings (relative 2^-23 per iteration), not always to the bit.
 * MRT_ERR_STATE without guides (as above) and on a sharded renderer (mrt_renderer_set_shard with world > 1): the filter needs its neighbours, and
 * assembling the guides of a device group is not provided.  MRT_ERR_INVALID_ARGUMENT for parameters out of range.                          */
typedef struct {
    int32_t iterations;     /* 1..8, default 5: step 1, 2, 4, ...                 */
    float   sigma_color;    /* > 0, on luminance of the filtered signal           */
    float   sigma_normal;   /* > 0, on 1 - max(0, n_p . n_q)                      */
    float   sigma_depth;    /* > 0, on |t_p - t_q| / (t_p * step)                 */
    int32_t demodulate;     /* 1 (default): filter colour / albedo, multiply back */
    int32_t _pad[3];
} MRTDenoiseParams;         /* 32 B; NULL = defaults                              */
#define MRT_DENOISE_DEFAULT_ITERATIONS   5
#define MRT_DENOISE_DEFAULT_SIGMA_COLOR  4.0f     /* chosen on the CPU restatement against a 512-frame image (DESIGN.md "Guide buffers and denoiser") */
#define MRT_DENOISE_DEFAULT_SIGMA_NORMAL 0.25f
#define MRT_DENOISE_DEFAULT_SIGMA_DEPTH  0.25f
int mrt_renderer_denoise(MRTRenderer r, const MRTDenoiseParams *params);
/* The denoised image of the last mrt_renderer_denoise (MRT_ERR_STATE before the first): w*h RGBA32F, row 0 = bottom, as mrt_renderer_read_accum. */
int mrt_renderer_read_denoised(MRTRenderer r, float *rgba, size_t nbytes);
int mrt_renderer_copy_denoised_to_device(MRTRenderer r, void *device_ptr, size_t nbytes);
/* mrt_renderer_read_tonemapped_rgba8 of the denoised image: what a host puts on screen.        */
int mrt_renderer_read_denoised_tonemapped_rgba8(MRTRenderer r, uint8_t *rgba, size_t nbytes);

/* Guide buffers, denoiser and tonemap as stages on DEVICE buffers, ordered on a stream of the caller's: the three steps above for an image the CALLER
 * holds — a frame composed from the stage entries, a torch tensor, the image mrt_group_gathered_device_ptr assembles — with no renderer in the loop.  None reads a scene.
 *   Common (the rules of the path-state entries): buffers are on the context's device and stay alive until the stream has passed the call; hip_stream is taken literally
 *     (0 is HIP's null stream); after the call nothing is allocated, nothing is copied from host memory and nothing waits.  Plain arguments are checked first, the message
 *     names the argument, and a NULL context is refused last.  Rows of 16 bytes are 16-byte aligned.  Arithmetic is float32, one rounding per operation, IEEE divide.
 *     Images are laid out like the accumulation buffer: width*height entries, row 0 = bottom.
 *   mrt_context_fold_guides_device: one frame folded into the three guide buffers from the frame's bounce-0 surface rows — d_surfaces is npixels x MRTSurface as
 *     mrt_scene_resolve_hits_device wrote them for the rays of mrt_renderer_primary_rays_device, row p = pixel p.  The outputs are laid out exactly as
 *     MRT_GUIDE_NORMAL_DEPTH / _ALBEDO / _IDS.  Per pixel: on = type == 1; n_new = on ? {normal, distance} : 0; a_new = on ? {base_color, 1} : 0;
 *     ids = on ? {1, instance_id, geometry_id, primitive_id} : {0, -1, -1, -1} — a row that is not on contributes these whatever its other words hold.
 *     frame_index == 0 replaces the averages (the old contents are not read: any bits are a valid start); otherwise (new + old * (float)frame_index) /
 *     (float)(frame_index + 1) per component, all four of both buffers.  The ids are always this frame's.  One kernel per call; npixels == 0 is MRT_OK and launches
 *     nothing.  Folding frames 0 .. f - 1 of a renderer's primary rays gives that renderer's guides after f frames, bit for bit.
 *     MRT_ERR_INVALID_ARGUMENT: npixels >= 2^31, frame_index == 2^32 - 1, a NULL or misaligned buffer with npixels > 0, two of the four buffers being the same pointer.
 *   mrt_context_denoise_device: exactly the filter mrt_renderer_denoise defines (the comment block above; params == NULL = the same defaults) with d_image in place of the
 *     accumulation buffer, d_workspace (mrt_denoise_workspace_bytes: two images, 2 * width * height * 16) in place of the two scratch images and d_out in place of the
 *     denoised buffer.  d_image.w is ignored; the output alpha is 1; the inputs are not modified.  MRT_ERR_INVALID_ARGUMENT: parameters out of range (as
 *     mrt_renderer_denoise), width or height <= 0, width * height >= 2^30, a NULL or misaligned buffer, workspace_bytes too small, d_out or the workspace overlapping an
 *     input or each other (byte ranges).
 *   mrt_context_tonemap_device: mrt_renderer_read_tonemapped_rgba8's image of d_image left on the device — Reinhard c / (1 + c), saturate,
 *     (unsigned char)(v * 255 + 0.5), alpha 255, rows flipped so the top row comes first.  d_rgba8 is width * height * 4 bytes, 4-byte aligned.  One kernel.
 *     MRT_ERR_INVALID_ARGUMENT: the sizes as above, a NULL or misaligned buffer, d_rgba8 overlapping d_image.
 * Guides and the filter for a device group: apply these entries to the gathered image on the root's context.                                                           */
int mrt_context_fold_guides_device(MRTContext ctx, size_t npixels, const void *d_surfaces, void *d_normal_depth, void *d_albedo, void *d_ids, uint32_t frame_index,
                                   void *hip_stream);
int mrt_denoise_workspace_bytes(int32_t width, int32_t height, size_t *bytes);
int mrt_context_denoise_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, const void *d_normal_depth, const void *d_albedo, void *d_workspace,
                               size_t workspace_bytes, void *d_out, const MRTDenoiseParams *params, void *hip_stream);
int mrt_context_tonemap_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, void *d_rgba8, void *hip_stream);

/* Temporal reprojection of the accumulated image on DEVICE buffers, ordered on a stream of the caller's: mrt_context_fold_sample_device averages pixel p
 * onto pixel p and so has to restart whenever a camera or an instance moves; this entry finds where each visible surface point was in the previous frame, fetches the
 * history there if it is the same surface, and keeps averaging — the temporal step of SVGF-style pipelines (Schied et al. 2017), without moments.  The common rules of
 * the image stages above hold: buffers of the context's device, hip_stream taken literally, ONE launch, nothing allocated, copied from host memory or waited for; plain
 * arguments checked first, each message naming its argument, a NULL context refused last; every refusal leaves d_out untouched.  Reads no scene.
 *   width, height     images are laid out like the accumulation buffer: pixel p = y * width + x, row 0 = bottom; npixels = width * height
 *   camera            this frame's camera and prev_camera the previous frame's, in HOST memory (copied into the launch)
 *   d_surfaces        npixels x MRTSurface, row p = pixel p: this frame's bounce-0 rows (mrt_scene_resolve_hits_device for mrt_renderer_primary_rays_device's rays)
 *   d_prev_position   npixels x 16 bytes, xyz used: the world position, IN THE PREVIOUS FRAME, of the surface point seen at p now.  NULL = the geometry did not move:
 *                     the row's own position is used.  The caller makes it (rigid instances: the two poses applied to the row's position; deformation:
 *                     mrt_scene_interpolate_device over the previous vertices); no entry here produces it.
 *   d_prev_normal_depth, d_prev_ids   float4 {n.xyz, t} and int4 {on, instance, geometry, primitive}: the PREVIOUS frame's own guide entries, not averaged — what
 *                     mrt_context_fold_guides_device(prev surfaces, frame_index = 0) wrote
 *   d_prev_history    float4: rgb = the accumulated colour, w = the history length in frames.  A zero-filled buffer is a valid "no history" start.
 *   d_sample          float4: this frame's radiance, w ignored
 *   d_out             float4: rgb = the new accumulated colour, w = the new history length — the next frame's d_prev_history
 *   params            NULL = the defaults below
 * The definition, per pixel (x, y): float32, one rounding per operation, no fused multiply-add, IEEE divide, no square root.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 * cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).
 *   project(C, q) inverts the ray generation (px = x + jitter; direction = normalize(((px / width) 2 - 1) right + ((py / height) 2 - 1) up + forward)) for any
 *     non-degenerate basis: nx = cross(up, forward), ny = cross(forward, right), nz = cross(right, up), det = dot(right, nx); v = q - C.position; a = dot(v, nx) / det,
 *     b = dot(v, ny) / det, c = dot(v, nz) / det.  It fails unless c > 0 (a NaN fails).  Otherwise px = ((a / c + 1) * 0.5) * (float)width, py = ((b / c + 1) * 0.5) *
 *     (float)height, d2 = dot(v, v).
 *   1. cur = d_surfaces[p].  cur.type != 1: out = {sample.rgb, 1}.
 *   2. P1 = project(camera, cur.position); P0 = project(prev_camera, prev_position).  Either fails or gives a px or py that is not finite: out = {sample.rgb, 1}.
 *   3. fx = (float)x + (P0.px - P1.px), fy = (float)y + (P0.py - P1.py) — the motion-vector form: the sub-pixel jitter of the primary ray cancels and a still world
 *      gives fx == x exactly.  x0 = floor(fx), ax = fx - x0; y0 = floor(fy), ay = fy - y0.
 *   4. Four taps (i, j) in the order (0,0), (1,0), (0,1), (1,1) at column x0 + i, row y0 + j with weight w = (i ? ax : 1 - ax) * (j ? ay : 1 - ay).  A tap of weight 0
 *      is not read.  A tap is inside iff its float column lies in [0, width - 1] and its float row in [0, height - 1], decided before any conversion to an integer.  A
 *      tap is VALID iff it is inside, ids.on == 1, ids.instance == cur.instance_id, ids.geometry == cur.geometry_id (the primitive is not compared: a point may cross
 *      a triangle edge), dot(prev_n, cur.normal) >= min_cos_normal, fabs(t_prev * t_prev - P0.d2) <= depth_tolerance * P0.d2, and history.w >= 1.  Valid taps add
 *      sw += w; sc += w * history.rgb; sl += w * history.w.  The words of a tap that is not valid are selected away, never computed with: a NaN there does not reach
 *      the output.
 *   5. sw > 0: hist = sc / sw, len = min(sl / sw + 1, max_history) (min(a, b) = a < b ? a : b), out = {(sample.rgb + hist * (len - 1)) / len, len}.  Otherwise
 *      out = {sample.rgb, 1}.
 * By construction: equal cameras and d_prev_position == NULL over frames 0 .. f - 1 give mrt_context_fold_sample_device's accumulation bit for bit in rgb as long as
 * max_history > f and every on-surface pixel's previous ids equal this frame's ((s + a f) / (f + 1), the same expression); a clamped max_history = M gives the
 * exponential average (s + a (M - 1)) / M; a zero d_prev_history gives the sample.
 * Not provided: the Renderer's own draws do not reproject; there is no variance or moments buffer; the previous normal is not rotated with a rotating instance (fast
 * rotation loses history: conservative); a pixel that misses restarts at its sample; nothing here produces d_prev_position.
 * MRT_ERR_INVALID_ARGUMENT: width or height <= 0 or >= 2^24, width * height >= 2^30, a NULL camera, a NULL or not 16-byte aligned buffer (d_prev_position may be NULL),
 * d_out overlapping any input (byte ranges), max_history < 1 or not finite, min_cos_normal or depth_tolerance NaN, depth_tolerance < 0.                              */
typedef struct {
    float   max_history;      /* >= 1, finite: the history length is clamped to it (the exponential average's window)            */
    float   min_cos_normal;   /* a tap's normal . this pixel's normal must reach it                                             */
    float   depth_tolerance;  /* >= 0, on SQUARED distance relative to the reprojected point's: 0.1 is about 5 % in distance     */
    int32_t _pad;
} MRTReprojectParams;         /* 16 B; NULL = defaults                                                                           */
#define MRT_REPROJECT_DEFAULT_MAX_HISTORY     32.0f    /* chosen on the CPU restatement against a converged image */
#define MRT_REPROJECT_DEFAULT_MIN_COS_NORMAL  0.9f
#define MRT_REPROJECT_DEFAULT_DEPTH_TOLERANCE 0.1f
int mrt_context_reproject_device(MRTContext ctx, int32_t width, int32_t height, const MRTCamera *camera, const MRTCamera *prev_camera, const void *d_surfaces,
                                 const void *d_prev_position, const void *d_prev_normal_depth, const void *d_prev_ids, const void *d_prev_history, const void *d_sample,
                                 void *d_out, const MRTReprojectParams *params, void *hip_stream);

/* Variance-guided a-trous filter on DEVICE buffers, with moments, ordered on a stream of the caller's: the spatial step of SVGF (Schied et al. 2017)
 * after the temporal one above.  mrt_context_denoise_device filters every pixel with one sigma_color / step, whatever its history; this filter measures the colour
 * difference of a tap in standard deviations of the pixel's own luminance, estimated from the two accumulated luminance moments where the history is long enough and
 * from the moments of the pixel's neighbourhood where it is not, and carries that variance through its levels.  The common rules of the image stages above hold: buffers
 * of the context's device, hip_stream taken literally, nothing allocated, copied from host memory or waited for; plain arguments checked first, each message naming its
 * argument, a NULL context refused last; every refusal leaves the outputs untouched.  Neither entry reads a scene.  Images are width * height entries of 16 bytes, pixel
 * p = y * width + x, row 0 = bottom.  Arithmetic: float32, one rounding per operation, no fused multiply-add, IEEE divide, correctly rounded sqrt.  k(x) = max(0, 1 - x),
 * max(a, b) = fmaxf, lum(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z, A_p = max(albedo_p.rgb, 1e-3) per channel if demodulate and albedo_p.w != 0, else 1 — the A of
 * mrt_renderer_denoise.
 *   The temporal accumulation of the moments is DEFINED as a second call of mrt_context_reproject_device on the same stream, with the same cameras, surfaces, previous
 *   guide entries, previous positions and parameters: d_sample = the image mrt_context_moments_sample_device wrote and d_prev_history = the previous frame's output of
 *   that same second call (zeros at the start).  Its output is {m1, m2, 0, len}: the reprojected first and second luminance moment, blended with the taps, weights and
 *   length of the colour's call.  No reprojection kernel is added.
 *   mrt_context_moments_sample_device: d_out_p = {l, l * l, 0, 0} with c = sample_p.rgb / A_p, l = lum(c); demodulate != 0 divides by the albedo.  sample_p.w is ignored.
 *     With the albedo buffer the filter is given, the moments are in the units of the signal the filter works on.  ONE kernel: one 16-byte load per input, one 16-byte store.
 *     MRT_ERR_INVALID_ARGUMENT: width or height <= 0, width * height >= 2^30, a NULL or not 16-byte aligned buffer, d_out overlapping an input (byte ranges).
 *   mrt_context_denoise_variance_device: d_image float4, rgb = the accumulated colour (mrt_context_reproject_device's output; w ignored); d_moments float4 {m1, m2, ., len}
 *     (the second call's output); d_normal_depth, d_albedo, d_workspace (mrt_denoise_workspace_bytes: two images), d_out, the order of the checks, the overlap rules and the
 *     1 + iterations launches exactly as mrt_context_denoise_device.  params == NULL = the MRT_DENOISE_DEFAULT_* values, but sigma_color is IN STANDARD DEVIATIONS and is not
 *     divided by the step.  The inputs are not modified; the output alpha is 1.
 *     A working entry is {I.rgb, v}, 16 bytes: the variance rides in the word where mrt_renderer_denoise keeps coverage.  A pixel that is not covered (albedo.w == 0) stores
 *     v = -1.  A tap is skipped iff its v < 0 or it lies outside the image.  A covered pixel's v is never negative: every v below ends in max(0, .) or is a sum of
 *     non-negative terms.  A pixel that is not covered is copied through every level to the bit and is never a tap; its d_out is image.rgb, alpha 1.  Skipped taps are
 *     branched over or selected away, never multiplied by 0: a NaN in an entry that is not covered or lies outside does not reach a covered output.
 *     Prepass: I_p = image_p.rgb / A_p.  Covered and len_p >= MRT_VARIANCE_MIN_HISTORY: v_p = max(0, m2 - m1 * m1).  Covered with a shorter history (a NaN len counts as
 *       shorter): the spatial estimate over the 7 x 7 window at distance 1, row-major from (-3, -3) — taps q inside the image with albedo_q.w != 0 take
 *       w = k(xn)^2 * k(xz)^2 with xn = (1 - max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)) / sigma_normal, xz = |t_p - t_q| / (sigma_depth * t_p), the centre takes
 *       w = 1;  s1 += w * m1_q; s2 += w * m2_q; sw += w;  M1 = s1 / sw, M2 = s2 / sw;  v_p = max(0, M2 - M1 * M1) * (4 / max(len_p, 1)) — SVGF's boost for young pixels.
 *     Iteration it (step = 1 << it), for a covered pixel p:
 *       1. g = the 3 x 3 Gaussian of v over the ADJACENT pixels, at distance 1 at every level: weights 1/4 centre, 1/8 edges, 1/16 corners; taps inside the image with
 *          v_q >= 0, row-major from (-1, -1): gs += weight * v_q; gw += weight;  g = gs / gw.
 *       2. den = sigma_color * sqrt(g) + MRT_VARIANCE_EPSILON.
 *       3. The 25 taps q = p + step * (dx, dy) in mrt_renderer_denoise's order with its h, xn and xz (xz = |t_p - t_q| / ((sigma_depth * t_p) * step)) and
 *          xc = |lum(I_p) - lum(I_q)| / den:  w = ((h * k(xn)^2) * k(xz)^2) * k(xc)^2, the centre takes w = h;  sum += w * I_q; vs += (w * w) * v_q; wsum += w.
 *       4. I'_p = sum / wsum, v'_p = vs / (wsum * wsum).
 *     The last iteration writes {I' * A_p, 1} to d_out.
 *     MRT_ERR_INVALID_ARGUMENT: as mrt_context_denoise_device, d_moments being a fourth input; and height > MRT_VARIANCE_MAX_HEIGHT — a workgroup of the prepass and of
 *     the larger steps covers 8 rows and a launch has at most 65535 workgroups in y.  (mrt_context_denoise_device has the same launch shape and no such check: an image
 *     taller than that fails there with MRT_ERR_HIP.)
 * Not provided: Renderer.draw does neither (mrt_renderer_denoise is the fixed-sigma filter); no stage makes d_prev_position; the first level's output is not fed back into
 * the colour history as SVGF does; the two reprojection calls of a frame are not fused into one launch.                                                                 */
#define MRT_VARIANCE_MIN_HISTORY 4.0f     /* frames of history from which a pixel's own two moments give its variance                     */
#define MRT_VARIANCE_MAX_HEIGHT  524280   /* 65535 * 8: the tallest image mrt_context_denoise_variance_device takes                      */
#define MRT_VARIANCE_EPSILON     1e-6f    /* added to sigma_color * sqrt(g): a pixel of variance 0 accepts taps of its own luminance only */
int mrt_context_moments_sample_device(MRTContext ctx, int32_t width, int32_t height, const void *d_sample, const void *d_albedo, int32_t demodulate, void *d_out,
                                      void *hip_stream);
int mrt_context_denoise_variance_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, const void *d_moments, const void *d_normal_depth,
                                        const void *d_albedo, void *d_workspace, size_t workspace_bytes, void *d_out, const MRTDenoiseParams *params, void *hip_stream);

/* ---------------------------------------------------------------- device group (multi-GPU, one process)
 * The reference creates ONE device and ONE queue (MTLCreateSystemDefaultDevice + makeCommandQueue, Renderer.swift:46-59); this is that
 * seam widened to the n GPUs of a node.  The scene and its BVH are replicated on every device; the image is sharded by 8x8 screen tile
 * (tile_id % n == rank); each device accumulates its frames locally; mrt_group_gather assembles the image with ONE reduce(sum) of the
 * RGBA32F buffer — ncclReduce over xGMI (RCCL is opened when a group of several distinct devices is created), or peer copies + add.
 * The assembled image is bit-identical to the single-device image.                                                                  */
int mrt_group_create(const int *device_ids, int32_t n, MRTGroup *out);
/* Destroy the group renderers of a group, and any scene made on one of its contexts (mrt_group_context), before the group: while any is alive
 * the call is refused — MRT_ERR_STATE, nothing is freed.                                                                                */
int mrt_group_destroy(MRTGroup g);
int mrt_group_size(MRTGroup g, int32_t *n);
int mrt_group_context(MRTGroup g, int32_t rank, MRTContext *ctx);                  /* borrowed: the group owns its contexts            */
/* mode: 0 = ncclReduce(sum, float32, root 0) of the whole buffers, 1 = peer copies of the whole buffers into the root device + add, 2 = compact: every rank packs the tiles it
 * owns (1 / n of the image) and the root receives them (ncclSend / ncclRecv, or peer copies) and writes them in place; note: why (may be NULL).  Same image bit for bit.        */
int mrt_group_reduce_mode(MRTGroup g, int32_t *mode, char *note, size_t note_len);
int mrt_group_set_reduce_mode(MRTGroup g, int32_t mode);
/* Renderer.init for the whole group: `scene` (any context; committed or not) is the template — its meshes, lights and build options are
 * replicated and committed on every device; rank r renders the tiles with tile_id % n == r.  The template scene stays the caller's.  */
int mrt_group_renderer_create(MRTGroup g, MRTScene scene, int32_t width, int32_t height, uint32_t seed, int32_t max_bounces, MRTGroupRenderer *out);
int mrt_group_renderer_destroy(MRTGroupRenderer gr);
int mrt_group_renderer_rank(MRTGroupRenderer gr, int32_t rank, MRTRenderer *r);     /* borrowed: one device's renderer (options, stats)  */
int mrt_group_set_option(MRTGroupRenderer gr, const char *key, double value);      /* mrt_renderer_set_option on every device           */
int mrt_group_set_camera(MRTGroupRenderer gr, const MRTCamera *camera);
/* draw(in:) (Renderer.swift:284-351) n_frames times on every device: enqueues and returns; the devices run concurrently.              */
int mrt_group_render(MRTGroupRenderer gr, int32_t n_frames);
int mrt_group_wait(MRTGroupRenderer gr);
int mrt_group_frames_completed(MRTGroupRenderer gr, uint64_t *frames);             /* minimum over the devices; never blocks            */
/* The one collective per output image: reduce(sum) of every device's accumulation buffer into rank 0, then (rgba != NULL) a copy of
 * the assembled w*h RGBA32F image to the host (row 0 = bottom, as mrt_renderer_read_accum).  Blocks until the image is assembled.   */
int mrt_group_gather(MRTGroupRenderer gr, float *rgba, size_t nbytes);
int mrt_group_gathered_device_ptr(MRTGroupRenderer gr, void **device_ptr);         /* the assembled image on the root device            */
int mrt_group_stats(MRTGroupRenderer gr, MRTRenderStats *out);                     /* ray counters summed over the devices              */

/* Diagnostics, device-function probes and the library-internal A/B switches (mrt_debug_*) are declared in mrt_debug.h — used by tests/,
 * tools/ and bench.py, not part of the host contract and not installed with this header.                                              */

#ifdef __cplusplus
}
#endif
#endif /* MRT_ABI_H */
