/* Episode debug log C ABI (csrc/dm_trace.hip, part of libdeepmimic_hip.so); Python side: deepmimic_mujoco_amd/debug_log.py.
 *
 * A per-env ring of the last K steps kept on the device (src/deepmimic_env.py:299,457-463: episode_debug_log), and frozen
 * copies of the rings of the envs whose step ended with a chosen reason (:366-378, :465-476).  The engines are not known here:
 * the caller hands in what their get_state entry points wrote.  All pointers are device pointers owned by the caller; every call
 * only enqueues kernels on `stream` (no host synchronisation: capturable into a hipGraph) and returns 0 or a negative code.
 */
#ifndef DEEPMIMIC_TRACE_H
#define DEEPMIMIC_TRACE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_TRACE_OK 0
#define DM_TRACE_EINVAL (-22) /* = DM_EINVAL of include/deepmimic_hip.h */
#define DM_TRACE_EHIP (-5)    /* = DM_EHIP */
#define DM_TRACE_TAIL 5       /* reward, done, reason, kind, step */
#define DM_TRACE_KIND_STEP 0  /* the state after a step, the action given to it, what it returned */
#define DM_TRACE_KIND_MARK 1  /* a state set from outside (reset, set_state, step_forced): zero action, reward, done, reason */

/* An entry is W = nq + 2 nv + na + 5 floats: qpos | qvel | qacc_warmstart | action | reward, done, reason, kind, step; the last
 * four are int32 bit patterns.  `step` is the env's entry count before this one.  Entry j of an env lives in row j mod K. */
typedef struct DmTraceBufs {
    int32_t N, K, C, nq, nv, na, W, device;
    float* ring;        /* [N, K, W] */
    uint32_t* head;     /* [N] entries ever written */
    float* cap;         /* [C, K, W] frozen rings, oldest entry first; rows and slots never written stay as the caller zeroed them */
    int32_t* cap_meta;  /* [C, 4] {env, valid entries, head at the trigger, reason} */
    int32_t* cap_count; /* [2] {copies filed (at most C), triggers seen} */
    int32_t* trig;      /* [N] scratch of one dm_trace_record call: zero between calls */
} DmTraceBufs;

/* One entry (kind 0) for every env of env_ids[0..nslots) (int32; NULL: envs 0..nslots-1, nslots = N; an entry outside [0, N) is
 * skipped; an env is listed at most once).  qpos [N,nq], qvel / warm [N,nv], actions [N,na], rew float[N], done uint8[N],
 * reason int32[N]: all indexed by env.  Then every listed env with done != 0 and bit `reason` set in reason_mask is a trigger:
 * the triggers of one call take the next free slots of cap in ascending env order and receive the env's ring, min(head, K)
 * rows; triggers beyond C are only counted.  Two launches. */
int dm_trace_record(const DmTraceBufs* bufs, const float* qpos, const float* qvel, const float* warm, const float* actions,
                    const float* rew, const uint8_t* done, const int32_t* reason, const int32_t* env_ids, int nslots,
                    uint32_t reason_mask, void* stream);

/* One entry of kind 1 for every listed env.  One launch. */
int dm_trace_mark(const DmTraceBufs* bufs, const float* qpos, const float* qvel, const float* warm, const int32_t* env_ids,
                  int nslots, void* stream);

/* Both return DM_TRACE_EINVAL before any HIP call for a NULL required pointer, N < 1, K < 2, C < 1, W != nq + 2 nv + na + 5 or
 * nslots outside [1, N]; the reason is kept per host thread. */
const char* dm_trace_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
