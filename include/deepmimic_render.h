/* Ray-cast renderer C ABI (csrc/dm_render.hip, part of libdeepmimic_hip.so); Python side: deepmimic_mujoco_amd/raycast.py.
 *
 * A scene is a set of flat tables made on the host (raycast.build_scene): the body tree with its free / hinge joints, the
 * rendered geoms (floor plane + every collision geom) and, per convex hull, one half-space (nx, ny, nz, d), n.x <= d, per
 * triangle in the mesh frame.  dm_render_create uploads them once.  All other pointers are device pointers; every call
 * only enqueues kernels on `stream` (capturable into a hipGraph) and returns 0, or a negative code with dm_render_last_error set.
 */
#ifndef DEEPMIMIC_RENDER_H
#define DEEPMIMIC_RENDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_RENDER_MAX_BODIES 64    /* per-lane body pose arrays of the kinematics kernel */
#define DM_RENDER_MAX_GEOMS 256    /* one lane per geom in the tile's bounding-sphere pass */
#define DM_RENDER_TILE 16          /* a workgroup casts a 16 x 16 pixel tile */
#define DM_RENDER_PLANE_CHUNK 1024 /* hull planes staged through LDS per round (16 KB of float4) */

/* geom types (mjtGeom numbering): 0 plane, 2 sphere, 3 capsule, 5 cylinder, 6 box, 7 convex hull; joint types: 0 free, 3 hinge */
typedef struct DmRenderSceneDesc {
    int32_t nq, nbody, njnt, ngeom, nplane, device;
    /* host pointers, copied by dm_render_create */
    const int32_t *body_parent, *body_jntadr, *body_jntnum;       /* [nbody] */
    const float *body_pos, *body_quat;                            /* [nbody,3] [nbody,4] (wxyz) */
    const int32_t *jnt_type, *jnt_qposadr;                        /* [njnt] */
    const float *jnt_axis, *jnt_pos, *jnt_ref;                    /* [njnt,3] [njnt,3] (anchor, body frame) [njnt] (qpos0 of a hinge) */
    const int32_t *geom_id, *geom_body, *geom_type, *geom_planeadr, *geom_planenum; /* [ngeom]; geom_id = the model's geom index */
    const float *geom_pos, *geom_quat, *geom_size, *geom_rbound, *geom_rgba;        /* [ngeom,3] [ngeom,4] [ngeom,3] [ngeom] [ngeom,4] */
    const float *planes;                                          /* [nplane,4] */
    float checker[6], sky[3], light[3];                           /* floor checker colours, miss colour, unit vector towards the light */
    float ambient, diffuse;                                       /* shade = ambient + diffuse * max(0, n . light) */
} DmRenderSceneDesc;

typedef void* DmRenderHandle;

int dm_render_create(const DmRenderSceneDesc* desc, DmRenderHandle* out);
int dm_render_destroy(DmRenderHandle h);
const char* dm_render_last_error(DmRenderHandle h); /* h may be NULL: the last create error */

/* qpos float[N*nq] as dm_get_state / dmg1_get_state write it; env_ids int32[n] rows of qpos, or NULL for rows 0..n-1.
 * Writes geom_xpos[n,ngeom,3] and geom_xmat[n,ngeom,9] (row-major, columns = geom axes in the world). */
int dm_render_kinematics(DmRenderHandle h, const float* qpos, const int32_t* env_ids, int n, float* geom_xpos, float* geom_xmat,
                         void* stream);

/* cam float[n*12]: eye, forward (unit), right * tan(fovy/2) * W/H, up * tan(fovy/2).  The ray of pixel (i, j) is
 * normalize(forward + (2(j+.5)/W-1) right + (1-2(i+.5)/H) up).  Any output may be NULL: rgb uint8[n,H,W,3];
 * depth float[n,H,W], metres along forward, +inf on a miss; seg int32[n,H,W], geom_id of the nearest hit, -1 on a miss. */
int dm_render_cast(DmRenderHandle h, const float* geom_xpos, const float* geom_xmat, int n, const float* cam, int W, int H,
                   uint8_t* rgb, float* depth, int32_t* seg, void* stream);

/* Both launches; workspace float[n*ngeom*12] holds the geom poses in between. */
int dm_render(DmRenderHandle h, const float* qpos, const int32_t* env_ids, int n, const float* cam, int W, int H, uint8_t* rgb,
              float* depth, int32_t* seg, float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
