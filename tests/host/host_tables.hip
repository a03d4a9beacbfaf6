// host_tables.hip — the two engines' host arithmetic (csrc/dm_tables_host.h, csrc/dm_g1_tables_host.h) on a CPU: no kernel, no
// HIP runtime call, so it runs under the host sanitizers (tests/test_host_tables_cpu.py builds it with them and runs it).
//
//   host_tables digest H_MODEL H_CLIP G1_MODEL G1_CLIP    check, build, hull clustering and clip packing of both robots; one line
//                                                         "<name> <64-bit FNV-1a, hex> <bytes>" per table
//   host_tables reject humanoid|g1 MODEL OFFSET:VALUE...  per case: the int32 at byte OFFSET of a copy of the model set to VALUE, the
//                                                         check function alone, one line "<rc> <message>"; nothing is built
// MODEL: the bytes of the model struct.  CLIP: int64 L, then qpos, qvel, body_xpos, geom_xpos of the L frames as doubles.
#include "../../deepmimic_mujoco_amd/csrc/dm_tables_host.h"
enum { H_NQ = DM_NQ, H_NV = DM_NV, H_NBODY = DM_NBODY, H_NGEOM = DM_NGEOM };
// include/dm_model.h once more, at the G1's dimensions (as dm_g1.hip sees it): DmModelG1
#undef DM_MODEL_H
#undef DM_NQ
#undef DM_NV
#undef DM_NU
#undef DM_NBODY
#undef DM_NGEOM
#undef DM_NJNT
#undef DM_NM
#undef DM_MAXPAIR
#undef DM_NOBS
#include "../../deepmimic_mujoco_amd/csrc/dm_g1_tables_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

static bool read_file(const char *path, std::vector<char> &out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize(n > 0 ? (size_t)n : 0);
  const bool ok = n >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}
struct Clip {
  std::vector<char> raw;
  int L = 0;
  const double *q = nullptr, *v = nullptr, *bx = nullptr, *gx = nullptr;
  bool load(const char *path, int nq, int nv, int nb, int ng) {
    if (!read_file(path, raw) || raw.size() < 8) return false;
    const int64_t L64 = *(const int64_t *)raw.data();
    if (L64 < 1 || raw.size() != 8 + (size_t)L64 * (nq + nv + 3 * nb + 3 * ng) * sizeof(double)) return false;
    L = (int)L64;
    q = (const double *)(raw.data() + 8); v = q + (size_t)L * nq; bx = v + (size_t)L * nv; gx = bx + (size_t)L * nb * 3;
    return true;
  }
};
static void digest(const char *name, const void *p, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < bytes; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  printf("%s %016llx %zu\n", name, (unsigned long long)h, bytes);
}
template <class T> static void digest(const char *name, const std::vector<T> &v) { digest(name, v.data(), v.size() * sizeof(T)); }

static int run_digest(char **a) {
  std::vector<char> hm, gm;
  Clip hc, gc;
  if (!read_file(a[0], hm) || hm.size() != sizeof(DmModel) || !hc.load(a[1], H_NQ, H_NV, H_NBODY, H_NGEOM) || !read_file(a[2], gm) ||
      gm.size() != sizeof(DmModelG1) || !gc.load(a[3], g1::NQ, g1::NV, g1::NB, g1::NG)) {
    fprintf(stderr, "host_tables: unreadable input or a size that is not the struct's\n");
    return 2;
  }
  std::string err;
  {
    const DmModel &m = *(const DmModel *)hm.data();
    if (check_model(m, err) != DM_OK) { fprintf(stderr, "check_model: %s\n", err.c_str()); return 1; }
    std::unique_ptr<DmDev> T(new DmDev);
    build_tables(m, *T);
    digest("humanoid_dev", T.get(), sizeof(DmDev));
    std::vector<float> rows((size_t)hc.L * DMK_CLIP_ROW, 0.f), reset((size_t)hc.L * DMK_RESET_ROW, 0.f);
    pack_clip(m, hc.L, hc.q, hc.v, hc.bx, hc.gx, rows.data(), reset.data());
    digest("humanoid_clip_rows", rows);
    digest("humanoid_reset_rows", reset);
  }
  {
    const DmModelG1 &m = *(const DmModelG1 *)gm.data();
    if (g1_check_model(m, err) != DM_OK) { fprintf(stderr, "g1_check_model: %s\n", err.c_str()); return 1; }
    std::unique_ptr<g1::Dev> T(new g1::Dev);
    g1_build_tables(m, *T);
    std::vector<double> verts, clus;
    std::vector<int32_t> oidx;
    if (g1_build_meshes(m, *T, verts, oidx, clus) != 0) { fprintf(stderr, "g1_build_meshes: too many clusters\n"); return 1; }
    digest("g1_dev", T.get(), sizeof(g1::Dev));
    digest("g1_verts", verts);
    digest("g1_oidx", oidx);
    digest("g1_clus", clus);
    std::vector<float> rows((size_t)gc.L * g1::CLIP_ROW, 0.f), reset((size_t)gc.L * g1::RESET_ROW, 0.f), com((size_t)gc.L * g1::COM_ROW, 0.f);
    g1_pack_clip(*T, gc.L, gc.q, gc.v, gc.bx, gc.gx, rows.data(), reset.data(), com.data());
    digest("g1_clip_rows", rows);
    digest("g1_reset_rows", reset);
    digest("g1_com_rows", com);
  }
  return 0;
}

static int run_reject(bool is_g1, const char *path, int ncase, char **cases) {
  std::vector<char> model;
  if (!read_file(path, model) || model.size() != (is_g1 ? sizeof(DmModelG1) : sizeof(DmModel))) {
    fprintf(stderr, "host_tables: unreadable model or a size that is not the struct's\n");
    return 2;
  }
  for (int c = 0; c < ncase; c++) {
    long off = -1;
    int value = 0;
    if (sscanf(cases[c], "%ld:%d", &off, &value) != 2 || off < 0 || off % 4 != 0 || (size_t)off + 4 > model.size()) {
      fprintf(stderr, "host_tables: bad case %s\n", cases[c]);
      return 2;
    }
    std::vector<char> edited(model);
    *(int32_t *)(edited.data() + off) = value;
    std::string err;
    const int rc = is_g1 ? g1_check_model(*(const DmModelG1 *)edited.data(), err) : check_model(*(const DmModel *)edited.data(), err);
    printf("%d %s\n", rc, err.c_str());
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "digest")) return run_digest(argv + 2);
  if (argc >= 4 && !strcmp(argv[1], "reject") && (!strcmp(argv[2], "humanoid") || !strcmp(argv[2], "g1")))
    return run_reject(!strcmp(argv[2], "g1"), argv[3], argc - 4, argv + 4);
  fprintf(stderr, "usage: host_tables digest H_MODEL H_CLIP G1_MODEL G1_CLIP | host_tables reject humanoid|g1 MODEL OFFSET:VALUE...\n");
  return 2;
}
