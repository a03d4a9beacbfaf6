// dm_host.h — the host layer both engines (dm_abi.hip, dm_g1.hip) stand on.  Host only, no kernels:
//   DmHost        base of an engine struct: its device, its error text, and every device buffer and event it owns
//   dm_fail       the one error helper; HIPCHK, DM_DEVICE, DM_LAUNCH: the checked-call, device-selection and launch idioms
//   the arithmetic the two table builders share, and the range check of a model's index fields (dm_range)
// The table builders (dm_tables_host.h, dm_g1_tables_host.h) use only the last group and call nothing from the HIP runtime.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#ifndef DM_OK   // include/deepmimic_hip.h has them for the humanoid engine
#define DM_OK 0
#define DM_EINVAL (-22)
#define DM_ENOMEM (-12)
#define DM_EHIP (-5)
#define DM_ENODEV (-19)
#endif

// Owns what an engine holds on its device.  Nothing is freed by name: a buffer or event made here dies with the engine.
struct DmHost {
  int device = 0;
  std::string err;   // dm_last_error / dmg1_last_error
  std::vector<void *> bufs;
  std::vector<hipEvent_t> events;

  DmHost() = default;
  DmHost(const DmHost &) = delete;
  DmHost &operator=(const DmHost &) = delete;
  ~DmHost() {
    if (bufs.empty() && events.empty()) return;   // refused before any device work: none now either
    (void)hipSetDevice(device);
    for (void *p : bufs) (void)hipFree(p);
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  }
  template <class T> hipError_t alloc(T **p, size_t count) {
    *p = nullptr;
    const hipError_t r = hipMalloc((void **)p, count * sizeof(T));
    if (r == hipSuccess && *p) bufs.push_back(*p);
    return r;
  }
  template <class T> hipError_t upload(T *dst, const T *src, size_t count) { return hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice); }
  hipError_t fill(void *dst, int byte, size_t bytes) { return hipMemset(dst, byte, bytes); }
  template <class T> void release(T *&p) {
    const auto it = std::find(bufs.begin(), bufs.end(), (void *)p);
    if (it != bufs.end()) { (void)hipFree(p); bufs.erase(it); }
    p = nullptr;
  }
  hipError_t event(hipEvent_t *ev) {
    const hipError_t r = hipEventCreate(ev);
    if (r == hipSuccess) events.push_back(*ev);
    return r;
  }
  // The tables of one clip slot, replaced together: the old ones go first, and a failure leaves every pointer null.
  hipError_t reload(std::initializer_list<std::pair<float **, const std::vector<float> *>> tables) {
    hipError_t r = hipSuccess;
    for (auto &t : tables) release(*t.first);
    for (auto &t : tables) {
      if (r == hipSuccess) r = alloc(t.first, t.second->size());
      if (r == hipSuccess) r = upload(*t.first, t.second->data(), t.second->size());
    }
    if (r != hipSuccess) for (auto &t : tables) release(*t.first);
    return r;
  }
};

static inline int dm_hip_code(hipError_t he) {
  return he == hipErrorOutOfMemory ? DM_ENOMEM : (he == hipErrorInvalidDevice || he == hipErrorNoDevice) ? DM_ENODEV : DM_EHIP;
}
static inline int dm_fail(DmHost *e, int code, const char *what, hipError_t he = hipSuccess) {
  if (e) {
    e->err = what;
    if (he != hipSuccess) { e->err += ": "; e->err += hipGetErrorString(he); }
  }
  return code;
}
#define HIPCHK(e, call)                                                \
  do {                                                                 \
    const hipError_t _r = (call);                                      \
    if (_r != hipSuccess) return dm_fail(e, dm_hip_code(_r), #call, _r); \
  } while (0)
// Every entry point that allocates, copies, launches, synchronizes or frees starts on its engine's device.
#define DM_DEVICE(e) HIPCHK(e, hipSetDevice((e)->device))
#define DM_LAUNCH(e, ...)               \
  do {                                  \
    hipLaunchKernelGGL(__VA_ARGS__);    \
    HIPCHK(e, hipGetLastError());       \
  } while (0)

static inline bool dm_have_device() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}
template <class E> static int dm_destroy_engine(E *e) {
  if (!e) return DM_EINVAL;
  hipError_t r = hipSetDevice(e->device);
  if (r == hipSuccess) r = hipDeviceSynchronize();
  delete e;   // ~DmHost frees the buffers and the events
  return r == hipSuccess ? DM_OK : DM_EHIP;
}
// The clips a launch needs: clip 0 always, and walk, run, getup under the combined task.  The message, or null.
static inline const char *dm_clips_missing(const int *L, bool combined, bool g1) {
  if (L[0] < 1) return g1 ? "no clip loaded (dmg1_load_clip clip 0 first)" : "no clip loaded (dm_load_clip clip 0 first)";
  if (combined && (L[1] < 1 || L[2] < 2)) return "combined task needs clips 0, 1, 2 = walk, run, getup";
  return nullptr;
}

// ------------------------------------------------------------------------------------------ shared model arithmetic
static inline void dm_quat_to_mat(const double *q, double *M) {   // wxyz -> row-major 3 x 3
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[9] = {w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z};
  for (int i = 0; i < 9; i++) M[i] = R[i];
}
// stiffness and damping of the reference acceleration from solref / solimp (refsafe applied)
static inline void dm_ref_kb(const double *solref, const double *solimp, double timestep, float &K, float &B) {
  const double tc = fmax(solref[0], 2 * timestep), dr = solref[1], dmax = solimp[1];
  K = (float)(1.0 / fmax(1e-15, dmax * dmax * tc * tc * dr * dr));
  B = (float)(2.0 / fmax(1e-15, dmax * tc));
}
// mass-weighted centre of one frame's body positions (nb x 3); the masses are summed in body order, in double
template <class M> static inline void dm_mass_centre(const M *mass, int nb, const double *xpos, double *out) {
  double mt = 0;
  for (int b = 0; b < nb; b++) mt += mass[b];
  for (int i = 0; i < 3; i++) {
    double c = 0;
    for (int b = 0; b < nb; b++) c += xpos[(size_t)b * 3 + i] * (double)mass[b];
    out[i] = c / mt;
  }
}

// DM_EINVAL and "<field> out of range" unless every v[i], i in [first, n), is in [lo, hi), or in [lo, i) with `precedes` (a tree's
// parent table: walking up from any entry ends)
static inline int dm_range(std::string &err, const char *field, const int32_t *v, int first, int n, int lo, int hi, bool precedes = false) {
  for (int i = first; i < n; i++)
    if (v[i] < lo || v[i] >= (precedes ? i : hi)) { err = std::string(field) + " out of range"; return DM_EINVAL; }
  return DM_OK;
}
static inline const int32_t *dm_ints(const int32_t &x) { return &x; }
template <size_t N> static inline const int32_t *dm_ints(const int32_t (&a)[N]) { return a; }
// inside a check function with the model `m` and the message `err` in scope
#define DM_RANGE(field, n, lo, hi) \
  do { if (dm_range(err, #field, dm_ints(m.field), 0, n, lo, hi) != DM_OK) return DM_EINVAL; } while (0)
#define DM_PRECEDES(field, first, n, lo) \
  do { if (dm_range(err, #field, dm_ints(m.field), first, n, lo, 0, true) != DM_OK) return DM_EINVAL; } while (0)
#define DM_REJECT(msg) return (err = (msg), DM_EINVAL)
