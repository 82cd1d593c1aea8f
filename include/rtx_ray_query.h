/*
 * rtx_ray_query.h — ray queries: the part of librtx_hip.so's C ABI that
 * answers the caller's own rays against a scene created with
 * rtx_scene_create (rtx.h).  A header of its own beside rtx.h: rtx.h is the
 * render boundary the reference-side adapter (rtx_traceui.h) is recorded
 * against byte for byte (tests/golden/ref_pins), and a query is no part of
 * that boundary.  Status codes, rtx_last_error and the scene handle are
 * rtx.h's.
 */
#ifndef RTX_RAY_QUERY_H_
#define RTX_RAY_QUERY_H_

#include "rtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Batched queries of the resident scene with the caller's own rays (what
 * RayTracer::traceRay-style probing, picking, visibility tests or light
 * baking need), answered by the traversal every render kernel runs.
 *   RTX_QUERY_CLOSEST : the closest hit of each ray (Scene::intersect,
 *                       scene/scene.cpp:157-180); kmax must be 1.
 *   RTX_QUERY_ALL     : every hit of each ray, ordered as the reference's
 *                       Scene::intersectList + std::sort leaves them
 *                       (scene/light.cpp:25-26) — the shadow walk's chain of
 *                       next-hit queries — truncated to the first kmax.
 * (The numbering is the CPU restatement's oracle_query_batch.)
 *   origins, dirs : [n][3] doubles, world space; directions are used as
 *                   given (not normalized).  A zero or non-finite direction
 *                   gets whatever the reference's arithmetic gives; the walk
 *                   is bounded by the tree either way.
 *   t, object, face : [n][kmax], each may be NULL.  Entry j of ray k is its
 *                   j-th hit: world t, RtxObject.orig_id, and for a trimesh hit
 *                   RtxFaceIds.orig_id of the face (-1 for other objects).
 *                   Unused entries are t = 0.0, object = face = -1.
 *   nhits         : [n], may be NULL: entries written for the ray (<= kmax).
 * With `device_ptrs` zero all arrays are host pointers and the call is
 * synchronous (staged through buffers the scene keeps and rtx_scene_destroy
 * frees); otherwise they are device (HBM) pointers and the work is enqueued
 * on `stream` (a hipStream_t, NULL = default stream), as in rtx_render.
 * Queries of one scene run one after the other whatever their streams (they
 * share a claim counter and stack scratch); calls for one scene must not be
 * made from two threads at once.
 * A query is independent of rendering: it touches no frame context, none of
 * rtx_kernel_time's counters, rtx_last_work or the frame history.
 * Errors: RTX_ERR_INVALID for a null scene, an unknown mode, n < 0,
 * kmax < 1, kmax != 1 with RTX_QUERY_CLOSEST, or null origins / dirs with
 * n > 0 (the arguments are checked before the scene is used);
 * RTX_ERR_CAPACITY for n above 2^31 or kmax above RTX_QUERY_KMAX.
 * n == 0 returns RTX_OK and launches nothing.
 * Out of scope: hit normals, uv or material; a per-ray tmax; shaded colours
 * for user rays; splitting a batch across GPUs. */
enum { RTX_QUERY_CLOSEST = 0, RTX_QUERY_ALL = 1 };
#define RTX_QUERY_KMAX 64
rtx_status rtx_query(void* scene, int32_t mode, int64_t n,
                     const double* origins, const double* dirs,
                     int32_t kmax,
                     double* t, int32_t* object, int32_t* face,
                     int32_t* nhits,
                     int device_ptrs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTX_RAY_QUERY_H_ */
