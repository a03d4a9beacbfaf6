// Ray-cast renderer (include/deepmimic_render.h): rgb, depth and segmentation frames of either robot from qpos alone.
//
//   render_kinematics_kernel   one lane per env walks the body tree (free + hinge joints) and writes the geom poses
//   render_cast_kernel         one 256-thread workgroup per 16 x 16 pixel tile of one env
//
// The cast kernel's barriers sit in loops whose trip counts are workgroup-uniform by construction: the candidate count is one
// LDS word written before a barrier and read back through readfirstlane, the geom of a round is an LDS word read the same way,
// and a hull's chunk count comes from geom_planenum[] at that uniform index.  No lane leaves early: a lane whose pixel is outside
// the image, or whose ray misses a hull's bounding sphere, runs every round and barrier and skips only arithmetic and stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/deepmimic_render.h"

namespace {

enum { OK = 0, EARG = -1, EHIP = -2 };
enum { G_PLANE = 0, G_SPHERE = 2, G_CAPSULE = 3, G_CYLINDER = 5, G_BOX = 6, G_HULL = 7, J_FREE = 0 };
constexpr int TILE = DM_RENDER_TILE, THREADS = TILE * TILE, CHUNK = DM_RENDER_PLANE_CHUNK;
constexpr float PARALLEL2 = 1e-12f;     // squared length of a direction's xy part below which it counts as parallel to z
constexpr float RB_REL = 1e-3f, RB_ABS = 1e-4f;   // bounding radii are inflated by this much before any culling test

struct Scene {   // device pointers
    int nq, nbody, njnt, ngeom, nplane;
    int *body_parent, *body_jntadr, *body_jntnum, *jnt_type, *jnt_qposadr;
    float *body_pos, *body_quat, *jnt_axis, *jnt_pos, *jnt_ref;
    int *geom_id, *geom_body, *geom_type, *geom_planeadr, *geom_planenum;
    float *geom_pos, *geom_quat, *geom_size, *geom_rbound, *geom_rgba;
    float4* planes;
    float checker[6], sky[3], light[3], ambient, diffuse;
};

struct Handle {
    Scene s;
    int device;
    void* slab;        // one allocation holds every table
    char err[256];
};

char g_create_err[256];

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 normalize(V3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }
__device__ __forceinline__ V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }

struct Q4 { float w, x, y, z; };
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
    return Q4{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
              a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
__device__ __forceinline__ Q4 qnormalize(Q4 q) {
    float s = 1.0f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    return Q4{q.w * s, q.x * s, q.y * s, q.z * s};
}
// row-major rotation matrix of a quaternion
__device__ __forceinline__ void qmat(Q4 q, float* m) {
    float w = q.w, x = q.x, y = q.y, z = q.z;
    m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
    m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
    m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ V3 mulv(const float* m, V3 v) {      // m v
    return v3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z);
}
__device__ __forceinline__ V3 mulTv(const float* m, V3 v) {     // m^T v
    return v3(m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z);
}

// ------------------------------------------------------------------------------------------------ kinematics
// The order of model.forward_kinematics: a body with one free joint takes its pose from qpos; any other body starts from its
// parent's pose times its own offset and turns about each hinge's anchor in turn.
__global__ __launch_bounds__(64) void render_kinematics_kernel(Scene s, const float* __restrict__ qpos, const int* __restrict__ env_ids,
                                                               int n, float* __restrict__ geom_xpos, float* __restrict__ geom_xmat) {
    int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* q = qpos + (size_t)(env_ids ? env_ids[i] : i) * s.nq;
    float xp[DM_RENDER_MAX_BODIES][3];
    Q4 xq[DM_RENDER_MAX_BODIES];
    xp[0][0] = xp[0][1] = xp[0][2] = 0.0f;
    xq[0] = Q4{1, 0, 0, 0};
    float m[9];
    for (int b = 1; b < s.nbody; ++b) {
        int p = s.body_parent[b], ja = s.body_jntadr[b], jn = s.body_jntnum[b];
        V3 pos;
        Q4 rot;
        if (jn == 1 && s.jnt_type[ja] == J_FREE) {
            const float* qa = q + s.jnt_qposadr[ja];
            pos = ld3(qa);
            rot = Q4{qa[3], qa[4], qa[5], qa[6]};
        } else {
            qmat(xq[p], m);
            pos = v3(xp[p][0], xp[p][1], xp[p][2]) + mulv(m, ld3(s.body_pos + 3 * b));
            const float* bq = s.body_quat + 4 * b;
            rot = qmul(xq[p], Q4{bq[0], bq[1], bq[2], bq[3]});
            for (int j = ja; j < ja + jn; ++j) {
                V3 jp = ld3(s.jnt_pos + 3 * j), ax = ld3(s.jnt_axis + 3 * j);
                qmat(rot, m);
                V3 anchor = mulv(m, jp) + pos;
                float half = 0.5f * (q[s.jnt_qposadr[j]] - s.jnt_ref[j]);
                float sn = sinf(half), cs = cosf(half);
                rot = qmul(rot, Q4{cs, ax.x * sn, ax.y * sn, ax.z * sn});
                qmat(rot, m);
                pos = anchor - mulv(m, jp);
            }
        }
        rot = qnormalize(rot);
        xp[b][0] = pos.x; xp[b][1] = pos.y; xp[b][2] = pos.z;
        xq[b] = rot;
    }
    for (int g = 0; g < s.ngeom; ++g) {
        int b = s.geom_body[g];
        qmat(xq[b], m);
        V3 gp = v3(xp[b][0], xp[b][1], xp[b][2]) + mulv(m, ld3(s.geom_pos + 3 * g));
        const float* gq = s.geom_quat + 4 * g;
        float gm[9];
        qmat(Q4{gq[0], gq[1], gq[2], gq[3]}, gm);
        float* op = geom_xpos + ((size_t)i * s.ngeom + g) * 3;
        float* om = geom_xmat + ((size_t)i * s.ngeom + g) * 9;
        op[0] = gp.x; op[1] = gp.y; op[2] = gp.z;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) om[3 * r + c] = m[3 * r] * gm[c] + m[3 * r + 1] * gm[3 + c] + m[3 * r + 2] * gm[6 + c];
    }
}

// ------------------------------------------------------------------------------------------------ intersections
// Every solid is convex, so a ray meets it in one interval [t_in, t_out]; it is hit iff t_in <= t_out and t_out > 0, at
// t = max(t_in, 0), with the normal of the surface that gave t_in.  The ray is o + t d in the geom frame, |d| = 1.
struct Hit { float tin, tout; V3 n; };

__device__ __forceinline__ bool sphere_interval(V3 o, V3 d, float r, float& t0, float& t1) {
    float b = dot(o, d);
    V3 p = o - b * d;                       // foot of the perpendicular from the centre
    float disc = r * r - dot(p, p);
    if (disc < 0.0f) return false;
    float sq = sqrtf(disc);
    t0 = -b - sq; t1 = -b + sq;
    return true;
}
// the infinite cylinder of radius r about z
__device__ __forceinline__ bool tube_interval(V3 o, V3 d, float r, float& t0, float& t1) {
    float a = d.x * d.x + d.y * d.y;
    if (a < PARALLEL2) {
        if (o.x * o.x + o.y * o.y > r * r) return false;
        t0 = -INFINITY; t1 = INFINITY;
        return true;
    }
    float b = (o.x * d.x + o.y * d.y) / a;
    float px = o.x - b * d.x, py = o.y - b * d.y;
    float disc = r * r - (px * px + py * py);
    if (disc < 0.0f) return false;
    float sq = sqrtf(disc / a);
    t0 = -b - sq; t1 = -b + sq;
    return true;
}
// the slab |x_axis| <= h; returns false on a miss; sets the entry normal sign through din
__device__ __forceinline__ bool slab_interval(float o, float d, float h, float& t0, float& t1) {
    if (d == 0.0f) {
        if (fabsf(o) > h) return false;
        t0 = -INFINITY; t1 = INFINITY;
        return true;
    }
    float a = (-h - o) / d, b = (h - o) / d;
    t0 = fminf(a, b); t1 = fmaxf(a, b);
    return true;
}

__device__ __forceinline__ bool hit_primitive(int type, V3 size, V3 o, V3 d, Hit& h) {
    float t0, t1;
    if (type == G_PLANE) {                  // one-sided: seen from above only
        if (!(d.z < 0.0f && o.z > 0.0f)) return false;
        h.tin = -o.z / d.z; h.tout = INFINITY; h.n = v3(0, 0, 1);
        return true;
    }
    if (type == G_SPHERE) {
        if (!sphere_interval(o, d, size.x, t0, t1)) return false;
        h.tin = t0; h.tout = t1; h.n = (1.0f / size.x) * (o + t0 * d);
        return true;
    }
    if (type == G_CAPSULE) {                // the union of a finite tube and two end spheres, itself convex
        float r = size.x, hl = size.y, lo = INFINITY, hi = -INFINITY, a0, a1, z0, z1;
        if (tube_interval(o, d, r, a0, a1) && slab_interval(o.z, d.z, hl, z0, z1)) {
            a0 = fmaxf(a0, z0); a1 = fminf(a1, z1);
            if (a0 <= a1) { lo = a0; hi = a1; }
        }
        if (sphere_interval(v3(o.x, o.y, o.z - hl), d, r, a0, a1)) { lo = fminf(lo, a0); hi = fmaxf(hi, a1); }
        if (sphere_interval(v3(o.x, o.y, o.z + hl), d, r, a0, a1)) { lo = fminf(lo, a0); hi = fmaxf(hi, a1); }
        if (lo > hi) return false;
        V3 p = o + lo * d;
        p.z -= fminf(fmaxf(p.z, -hl), hl);
        h.tin = lo; h.tout = hi; h.n = (1.0f / r) * p;
        return true;
    }
    if (type == G_CYLINDER) {
        float a0, a1, z0, z1;
        if (!tube_interval(o, d, size.x, a0, a1) || !slab_interval(o.z, d.z, size.y, z0, z1)) return false;
        h.tin = fmaxf(a0, z0); h.tout = fminf(a1, z1);
        if (z0 > a0) h.n = v3(0, 0, d.z > 0.0f ? -1.0f : 1.0f);
        else h.n = (1.0f / size.x) * v3(o.x + a0 * d.x, o.y + a0 * d.y, 0.0f);
        return h.tin <= h.tout;
    }
    if (type == G_BOX) {
        float x0, x1, y0, y1, z0, z1;
        if (!slab_interval(o.x, d.x, size.x, x0, x1) || !slab_interval(o.y, d.y, size.y, y0, y1) ||
            !slab_interval(o.z, d.z, size.z, z0, z1)) return false;
        h.tin = x0; h.n = v3(d.x > 0.0f ? -1.0f : 1.0f, 0, 0);
        if (y0 > h.tin) { h.tin = y0; h.n = v3(0, d.y > 0.0f ? -1.0f : 1.0f, 0); }
        if (z0 > h.tin) { h.tin = z0; h.n = v3(0, 0, d.z > 0.0f ? -1.0f : 1.0f); }
        h.tout = fminf(x1, fminf(y1, z1));
        return h.tin <= h.tout;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------ cast
__global__ __launch_bounds__(THREADS) void render_cast_kernel(Scene s, const float* __restrict__ geom_xpos, const float* __restrict__ geom_xmat,
                                                              const float* __restrict__ cam, int W, int H, unsigned char* __restrict__ rgb,
                                                              float* __restrict__ depth, int* __restrict__ seg) {
    __shared__ float4 s_planes[CHUNK];
    __shared__ float s_pose[DM_RENDER_MAX_GEOMS][12];
    __shared__ int s_cand[DM_RENDER_MAX_GEOMS];
    __shared__ int s_wcnt[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, env = blockIdx.z;
    const int px = blockIdx.x * TILE + (tid & (TILE - 1)), py = blockIdx.y * TILE + (tid / TILE);
    const bool inside = px < W && py < H;
    const float* cm = cam + (size_t)env * 12;
    const V3 eye = ld3(cm), fwd = ld3(cm + 3), right = ld3(cm + 6), up = ld3(cm + 9);

    // ---- phase 1: lane g tests geom g's bounding sphere against the cone of the tile's rays
    {
        float u0 = 2.0f * (blockIdx.x * TILE) / W - 1.0f, u1 = 2.0f * (blockIdx.x * TILE + TILE) / W - 1.0f;
        float v0 = 1.0f - 2.0f * (blockIdx.y * TILE) / H, v1 = 1.0f - 2.0f * (blockIdx.y * TILE + TILE) / H;
        V3 axis = normalize(fwd + (0.5f * (u0 + u1)) * right + (0.5f * (v0 + v1)) * up);
        // a rectangle of the image plane lies inside a circular cone iff its corners do
        float cos_t = fminf(fminf(dot(axis, normalize(fwd + u0 * right + v0 * up)), dot(axis, normalize(fwd + u1 * right + v0 * up))),
                            fminf(dot(axis, normalize(fwd + u0 * right + v1 * up)), dot(axis, normalize(fwd + u1 * right + v1 * up))));
        cos_t = fmaxf(cos_t - 1e-6f, 0.0f);
        float sin_t = sqrtf(1.0f - cos_t * cos_t);
        bool pass = false;
        if (tid < s.ngeom) {
            const float* gp = geom_xpos + ((size_t)env * s.ngeom + tid) * 3;
            const float* gm = geom_xmat + ((size_t)env * s.ngeom + tid) * 9;
            for (int k = 0; k < 3; ++k) s_pose[tid][k] = gp[k];
            for (int k = 0; k < 9; ++k) s_pose[tid][3 + k] = gm[k];
            if (s.geom_type[tid] == G_PLANE) {
                pass = true;
            } else {
                float r = s.geom_rbound[tid] * (1.0f + RB_REL) + RB_ABS;
                V3 v = ld3(gp) - eye;
                float dist = sqrtf(dot(v, v));
                if (dist <= r) {
                    pass = true;
                } else {
                    float sin_a = r / dist, cos_a = sqrtf(1.0f - sin_a * sin_a);
                    pass = dot(v, axis) >= dist * (cos_t * cos_a - sin_t * sin_a) - 1e-6f * dist;   // angle to the axis <= t + a < pi
                }
            }
        }
        unsigned long long m = __ballot(pass);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += s_wcnt[w];
        if (pass) s_cand[off + __popcll(m & ((1ull << lane) - 1ull))] = tid;      // ascending geom order
        __syncthreads();
    }
    const int ncand = __builtin_amdgcn_readfirstlane(s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3]);

    // ---- phase 2: every lane walks the same list
    float u = 2.0f * (px + 0.5f) / W - 1.0f, v = 1.0f - 2.0f * (py + 0.5f) / H;
    const V3 dir = normalize(fwd + u * right + v * up);
    float best = INFINITY;
    int best_g = -1;
    V3 best_n = v3(0, 0, 0);
    for (int ci = 0; ci < ncand; ++ci) {
        const int g = __builtin_amdgcn_readfirstlane(s_cand[ci]);
        const int type = s.geom_type[g];
        const float* pose = s_pose[g];
        V3 o = mulTv(pose + 3, eye - ld3(pose)), d = mulTv(pose + 3, dir);
        Hit h;
        bool hit;
        if (type != G_HULL) {
            hit = inside && hit_primitive(type, ld3(s.geom_size + 3 * g), o, d, h);
        } else {
            const int np = s.geom_planenum[g], adr = s.geom_planeadr[g];
            float r = s.geom_rbound[g] * (1.0f + RB_REL) + RB_ABS, b = dot(o, d);
            bool live = inside && dot(o, o) - b * b <= r * r;       // the ray's line comes within the bounding sphere
            h.tin = -INFINITY; h.tout = INFINITY; h.n = -1.0f * d;
            for (int c0 = 0; c0 < np; c0 += CHUNK) {                // np is uniform: every lane runs every round
                const int cnt = min(CHUNK, np - c0);
                __syncthreads();                                     // the previous round's planes have been read
                for (int k = tid; k < cnt; k += THREADS) s_planes[k] = s.planes[adr + c0 + k];
                __syncthreads();
                if (live) {
                    for (int k = 0; k < cnt; ++k) {
                        float4 p = s_planes[k];
                        float den = p.x * d.x + p.y * d.y + p.z * d.z;
                        float num = p.w - (p.x * o.x + p.y * o.y + p.z * o.z);
                        if (den < 0.0f) {
                            float t = num / den;
                            if (t > h.tin) { h.tin = t; h.n = v3(p.x, p.y, p.z); }
                        } else if (den > 0.0f) {
                            h.tout = fminf(h.tout, num / den);
                        } else if (num < 0.0f) {
                            h.tout = -INFINITY;                      // parallel to the plane and outside it
                        }
                    }
                }
            }
            hit = live && h.tin <= h.tout;
        }
        if (hit && h.tout > 0.0f) {
            float t = fmaxf(h.tin, 0.0f);
            if (t < best) {                                          // strict: equal t stays with the lower geom
                best = t; best_g = g; best_n = mulv(pose + 3, h.n);
            }
        }
    }

    if (!inside) return;                                             // after the last barrier
    size_t pix = ((size_t)env * H + py) * W + px;
    if (seg) seg[pix] = best_g < 0 ? -1 : s.geom_id[best_g];
    if (depth) depth[pix] = best_g < 0 ? INFINITY : best * dot(dir, fwd);
    if (rgb) {
        float cr = s.sky[0], cg = s.sky[1], cb = s.sky[2];
        if (best_g >= 0) {
            const float* col = s.geom_rgba + 4 * best_g;
            if (s.geom_type[best_g] == G_PLANE) {                    // 1 m checker in world x, y
                V3 p = eye + best * dir;
                col = s.checker + 3 * (((int)floorf(p.x) + (int)floorf(p.y)) & 1);
            }
            float shade = s.ambient + s.diffuse * fmaxf(0.0f, best_n.x * s.light[0] + best_n.y * s.light[1] + best_n.z * s.light[2]);
            cr = col[0] * shade; cg = col[1] * shade; cb = col[2] * shade;
        }
        unsigned char* out = rgb + pix * 3;
        out[0] = (unsigned char)(fminf(fmaxf(cr, 0.0f), 1.0f) * 255.0f + 0.5f);
        out[1] = (unsigned char)(fminf(fmaxf(cg, 0.0f), 1.0f) * 255.0f + 0.5f);
        out[2] = (unsigned char)(fminf(fmaxf(cb, 0.0f), 1.0f) * 255.0f + 0.5f);
    }
}

int fail(Handle* h, int code, const char* msg) {
    snprintf(h ? h->err : g_create_err, 256, "%s", msg);
    return code;
}

int launch_kinematics(Handle* h, const float* qpos, const int32_t* env_ids, int n, float* xpos, float* xmat, hipStream_t st) {
    hipLaunchKernelGGL(render_kinematics_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h->s, qpos, env_ids, n, xpos, xmat);
    return hipGetLastError() == hipSuccess ? OK : fail(h, EHIP, "render_kinematics_kernel launch refused");
}

int launch_cast(Handle* h, const float* xpos, const float* xmat, int n, const float* cam, int W, int H, uint8_t* rgb, float* depth,
                int32_t* seg, hipStream_t st) {
    dim3 grid((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, n);
    hipLaunchKernelGGL(render_cast_kernel, grid, dim3(THREADS), 0, st, h->s, xpos, xmat, cam, W, H, rgb, depth, seg);
    return hipGetLastError() == hipSuccess ? OK : fail(h, EHIP, "render_cast_kernel launch refused");
}

bool frame_ok(int n, int W, int H) { return n >= 1 && n <= 65535 && W >= 1 && H >= 1 && W <= 16384 && H <= 16384; }

}  // namespace

extern "C" {

int dm_render_create(const DmRenderSceneDesc* d, DmRenderHandle* out) {
    if (!d || !out) return fail(nullptr, EARG, "null argument");
    if (d->nbody < 1 || d->nbody > DM_RENDER_MAX_BODIES || d->ngeom < 1 || d->ngeom > DM_RENDER_MAX_GEOMS || d->njnt < 0 || d->nplane < 0 ||
        d->nq < 0)
        return fail(nullptr, EARG, "scene dimensions out of range");
    for (int j = 0; j < d->njnt; ++j) {
        int need = d->jnt_type[j] == J_FREE ? 7 : 1;
        if ((d->jnt_type[j] != J_FREE && d->jnt_type[j] != 3) || d->jnt_qposadr[j] < 0 || d->jnt_qposadr[j] + need > d->nq)
            return fail(nullptr, EARG, "joint table: only free and hinge joints inside qpos");
    }
    for (int b = 0; b < d->nbody; ++b)
        if (d->body_parent[b] < 0 || d->body_parent[b] > b || (b > 0 && d->body_parent[b] == b) ||
            (d->body_jntnum[b] > 0 && (d->body_jntadr[b] < 0 || d->body_jntadr[b] + d->body_jntnum[b] > d->njnt)))
            return fail(nullptr, EARG, "body table: parents must precede children, joints must be in range");
    for (int g = 0; g < d->ngeom; ++g) {
        int t = d->geom_type[g];
        if (d->geom_body[g] < 0 || d->geom_body[g] >= d->nbody || (t != G_PLANE && t != G_SPHERE && t != G_CAPSULE && t != G_CYLINDER &&
                                                                   t != G_BOX && t != G_HULL))
            return fail(nullptr, EARG, "geom table: body or type out of range");
        if (t == G_HULL && (d->geom_planeadr[g] < 0 || d->geom_planenum[g] < 1 || d->geom_planeadr[g] + d->geom_planenum[g] > d->nplane))
            return fail(nullptr, EARG, "geom table: hull planes out of range");
    }
    if (hipSetDevice(d->device) != hipSuccess) return fail(nullptr, EHIP, "hipSetDevice failed");
    Handle* h = new Handle();
    memset(h, 0, sizeof(*h));
    h->device = d->device;
    Scene& s = h->s;
    s.nq = d->nq; s.nbody = d->nbody; s.njnt = d->njnt; s.ngeom = d->ngeom; s.nplane = d->nplane;
    memcpy(s.checker, d->checker, sizeof(s.checker));
    memcpy(s.sky, d->sky, sizeof(s.sky));
    memcpy(s.light, d->light, sizeof(s.light));
    s.ambient = d->ambient; s.diffuse = d->diffuse;
    const int nb = d->nbody, nj = d->njnt > 0 ? d->njnt : 1, ng = d->ngeom, np = d->nplane > 0 ? d->nplane : 1;
    struct Item { void** dst; const void* src; size_t bytes; };
    const Item items[] = {
        {(void**)&s.planes, d->planes, sizeof(float) * 4 * (size_t)d->nplane},
        {(void**)&s.body_parent, d->body_parent, sizeof(int) * nb}, {(void**)&s.body_jntadr, d->body_jntadr, sizeof(int) * nb},
        {(void**)&s.body_jntnum, d->body_jntnum, sizeof(int) * nb}, {(void**)&s.body_pos, d->body_pos, sizeof(float) * 3 * nb},
        {(void**)&s.body_quat, d->body_quat, sizeof(float) * 4 * nb}, {(void**)&s.jnt_type, d->jnt_type, sizeof(int) * d->njnt},
        {(void**)&s.jnt_qposadr, d->jnt_qposadr, sizeof(int) * d->njnt}, {(void**)&s.jnt_axis, d->jnt_axis, sizeof(float) * 3 * d->njnt},
        {(void**)&s.jnt_pos, d->jnt_pos, sizeof(float) * 3 * d->njnt}, {(void**)&s.jnt_ref, d->jnt_ref, sizeof(float) * d->njnt},
        {(void**)&s.geom_id, d->geom_id, sizeof(int) * ng}, {(void**)&s.geom_body, d->geom_body, sizeof(int) * ng},
        {(void**)&s.geom_type, d->geom_type, sizeof(int) * ng}, {(void**)&s.geom_planeadr, d->geom_planeadr, sizeof(int) * ng},
        {(void**)&s.geom_planenum, d->geom_planenum, sizeof(int) * ng}, {(void**)&s.geom_pos, d->geom_pos, sizeof(float) * 3 * ng},
        {(void**)&s.geom_quat, d->geom_quat, sizeof(float) * 4 * ng}, {(void**)&s.geom_size, d->geom_size, sizeof(float) * 3 * ng},
        {(void**)&s.geom_rbound, d->geom_rbound, sizeof(float) * ng}, {(void**)&s.geom_rgba, d->geom_rgba, sizeof(float) * 4 * ng},
    };
    (void)nj; (void)np;
    size_t total = 0;
    for (const Item& it : items) total += (it.bytes + 255) & ~(size_t)255;
    if (hipMalloc(&h->slab, total + 256) != hipSuccess) {
        delete h;
        return fail(nullptr, EHIP, "hipMalloc of the scene tables failed");
    }
    size_t at = 0;
    for (const Item& it : items) {
        *it.dst = (char*)h->slab + at;
        if (it.bytes && hipMemcpy(*it.dst, it.src, it.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(h->slab);
            delete h;
            return fail(nullptr, EHIP, "upload of the scene tables failed");
        }
        at += (it.bytes + 255) & ~(size_t)255;
    }
    *out = h;
    return OK;
}

int dm_render_destroy(DmRenderHandle hv) {
    Handle* h = (Handle*)hv;
    if (!h) return OK;
    hipFree(h->slab);
    delete h;
    return OK;
}

const char* dm_render_last_error(DmRenderHandle hv) { return hv ? ((Handle*)hv)->err : g_create_err; }

int dm_render_kinematics(DmRenderHandle hv, const float* qpos, const int32_t* env_ids, int n, float* geom_xpos, float* geom_xmat,
                         void* stream) {
    Handle* h = (Handle*)hv;
    if (!h) return EARG;
    if (!qpos || !geom_xpos || !geom_xmat || n < 1) return fail(h, EARG, "dm_render_kinematics: null pointer or n < 1");
    return launch_kinematics(h, qpos, env_ids, n, geom_xpos, geom_xmat, (hipStream_t)stream);
}

int dm_render_cast(DmRenderHandle hv, const float* geom_xpos, const float* geom_xmat, int n, const float* cam, int W, int H, uint8_t* rgb,
                   float* depth, int32_t* seg, void* stream) {
    Handle* h = (Handle*)hv;
    if (!h) return EARG;
    if (!geom_xpos || !geom_xmat || !cam || !frame_ok(n, W, H)) return fail(h, EARG, "dm_render_cast: null pointer or frame out of range");
    return launch_cast(h, geom_xpos, geom_xmat, n, cam, W, H, rgb, depth, seg, (hipStream_t)stream);
}

int dm_render(DmRenderHandle hv, const float* qpos, const int32_t* env_ids, int n, const float* cam, int W, int H, uint8_t* rgb, float* depth,
              int32_t* seg, float* workspace, void* stream) {
    Handle* h = (Handle*)hv;
    if (!h) return EARG;
    if (!qpos || !cam || !workspace || !frame_ok(n, W, H)) return fail(h, EARG, "dm_render: null pointer or frame out of range");
    float* xpos = workspace;
    float* xmat = workspace + (size_t)n * h->s.ngeom * 3;
    int rc = launch_kinematics(h, qpos, env_ids, n, xpos, xmat, (hipStream_t)stream);
    return rc != OK ? rc : launch_cast(h, xpos, xmat, n, cam, W, H, rgb, depth, seg, (hipStream_t)stream);
}

}  // extern "C"
