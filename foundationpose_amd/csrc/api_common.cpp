// Error plumbing, mesh handles and the host-side cluster_poses and mesh_pseudonormals of libfp_amd.so.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "fp_common.h"

static thread_local char g_err[512] = "";

void fp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* fp_last_error(void) { return g_err; }
extern "C" int fp_version(void) { return FP_AMD_ABI_VERSION; }

extern "C" int fp_mesh_create(const float* pos, const float* nrm, const int32_t* faces, const float* uv,
                              const int32_t* uv_idx, const float* tex, const float* vcol, int V, int T, int Ht,
                              int Wt, fp_mesh** out) {
  FP_REQUIRE(out != nullptr, "fp_mesh_create: out is NULL");
  FP_REQUIRE(pos && nrm && faces, "fp_mesh_create: pos/nrm/faces are required");
  FP_REQUIRE(V > 0 && T > 0, "fp_mesh_create: empty mesh (V=%d, T=%d)", V, T);
  FP_REQUIRE((tex && uv && Ht > 0 && Wt > 0) || vcol, "fp_mesh_create: need (tex, uv) or vcol");
  fp_mesh* m = (fp_mesh*)calloc(1, sizeof(fp_mesh));
  m->pos = pos; m->nrm = nrm; m->faces = faces;
  m->uv = tex ? uv : nullptr;
  m->uv_idx = tex ? uv_idx : nullptr;
  m->tex = tex;
  m->vcol = tex ? nullptr : vcol;
  m->V = V; m->T = T; m->Ht = tex ? Ht : 0; m->Wt = tex ? Wt : 0;
  *out = m;
  return FP_OK;
}

extern "C" void fp_mesh_destroy(fp_mesh* mesh) { free(mesh); }

extern "C" int fp_mesh_set_create(const fp_mesh* const* meshes, int M, fp_mesh_set** out) {
  FP_REQUIRE(out != nullptr, "fp_mesh_set_create: out is NULL");
  *out = nullptr;
  FP_REQUIRE(M >= 1, "fp_mesh_set_create: empty set (M=%d)", M);
  FP_REQUIRE(meshes != nullptr, "fp_mesh_set_create: meshes is NULL");
  int maxV = 0, maxT = 0;
  for (int i = 0; i < M; ++i) {
    FP_REQUIRE(meshes[i] != nullptr, "fp_mesh_set_create: mesh %d is NULL", i);
    const int V = meshes[i]->V, T = meshes[i]->T;
    FP_REQUIRE(V > 0 && T > 0 && V <= FP_MESH_SET_MAX_ELEMS && T <= FP_MESH_SET_MAX_ELEMS,
               "fp_mesh_set_create: mesh %d has V=%d, T=%d (each must be in 1..%d)", i, V, T, FP_MESH_SET_MAX_ELEMS);
    maxV = V > maxV ? V : maxV;
    maxT = T > maxT ? T : maxT;
  }
  fp_mesh* host = (fp_mesh*)malloc(sizeof(fp_mesh) * (size_t)M);
  if (!host) {
    fp_set_error("fp_mesh_set_create: out of host memory");
    return FP_ERR_INVALID_ARG;
  }
  for (int i = 0; i < M; ++i) host[i] = *meshes[i];
  fp_mesh* dev = nullptr;
  hipError_t e = hipMalloc((void**)&dev, sizeof(fp_mesh) * (size_t)M);
  if (e == hipSuccess) e = hipMemcpy(dev, host, sizeof(fp_mesh) * (size_t)M, hipMemcpyHostToDevice);
  free(host);
  if (e != hipSuccess) {
    if (dev) (void)hipFree(dev);
    fp_set_error("fp_mesh_set_create: device table of %d meshes: %s", M, hipGetErrorString(e));
    return FP_ERR_LAUNCH;
  }
  fp_mesh_set* s = (fp_mesh_set*)calloc(1, sizeof(fp_mesh_set));
  s->meshes = dev;
  s->M = M; s->maxV = maxV; s->maxT = maxT;
  *out = s;
  return FP_OK;
}

extern "C" void fp_mesh_set_destroy(fp_mesh_set* set) {
  if (!set) return;
  if (set->meshes) (void)hipFree(set->meshes);
  free(set);
}

// Greedy symmetry-aware pose clustering (reference: mycpp/src/app/pybind_api.cpp:24-68,
// geodesic distance mycpp/src/Utils.cpp:21-26).  Init-time, O(N^2 S), host only.
extern "C" int fp_cluster_poses(float angle_diff_deg, float dist_diff, const float* poses, int N,
                                const float* sym, int S, int* keep_idx) {
  if (N <= 0) return 0;
  FP_REQUIRE(poses && sym && keep_idx && S > 0, "fp_cluster_poses: bad arguments");
  const float thres = (float)(angle_diff_deg / 180.0 * M_PI);
  int kept = 0;
  keep_idx[kept++] = 0;
  for (int i = 1; i < N; ++i) {
    const float* P = poses + (size_t)i * 16;
    bool fresh = true;
    for (int k = 0; k < kept && fresh; ++k) {
      const float* Q = poses + (size_t)keep_idx[k] * 16;
      const float ex = Q[3] - P[3], ey = Q[7] - P[7], ez = Q[11] - P[11];
      if (sqrtf((ex * ex + ey * ey) + ez * ez) >= dist_diff) continue;
      for (int s = 0; s < S; ++s) {
        const float* G = sym + (size_t)s * 16;
        float tr = 0.f;  // trace((P*G)_rot * Q_rot^T)
        for (int r = 0; r < 3; ++r) {
          float row[3];
          for (int c = 0; c < 3; ++c)
            row[c] = ((P[r * 4] * G[c] + P[r * 4 + 1] * G[4 + c]) + P[r * 4 + 2] * G[8 + c]) + P[r * 4 + 3] * G[12 + c];
          tr += (row[0] * Q[r * 4] + row[1] * Q[r * 4 + 1]) + row[2] * Q[r * 4 + 2];
        }
        float cs = fmaxf(fminf((tr - 1.0f) / 2.0f, 1.0f), -1.0f);
        if (acosf(cs) < thres) { fresh = false; break; }
      }
    }
    if (fresh) keep_idx[kept++] = i;
  }
  return kept;
}

// The angle-weighted pseudonormals of a mesh's vertices and edges and a report of its topology (include/fp_amd.h has the definition;
// Baerentzen and Aanaes 2005).  Setup-time, host only, float64 throughout, O((Nv + F) log).  Adjacency goes by vertex position: the
// indices whose three float32 coordinates compare equal (-0 == +0; a NaN equals nothing) are one vertex, named by the smallest of them.
namespace {

struct EdgeUse {
  unsigned long long key;   // (smaller welded index << 32) | larger
  int face;
  bool forward;             // traversed from the smaller welded index to the larger
};

inline unsigned ordered_bits(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  return (u << 1) == 0 ? 0u : u;   // -0 -> +0
}

}  // namespace

extern "C" int fp_mesh_pseudonormals(const float* pos, int Nv, const int32_t* faces, int F, float* vn, float* en, int32_t* report) {
  const char* name = "fp_mesh_pseudonormals";
  FP_REQUIRE(Nv >= 0 && Nv <= (1 << 30), "%s: Nv=%d outside 0..2^30", name, Nv);
  FP_REQUIRE(F >= 0 && F <= (1 << 30), "%s: F=%d outside 0..2^30", name, F);
  FP_REQUIRE(report, "%s: NULL report", name);
  FP_REQUIRE(Nv == 0 || (pos && vn), "%s: NULL pos or vn with Nv=%d", name, Nv);
  FP_REQUIRE(F == 0 || (faces && en), "%s: NULL faces or en with F=%d", name, F);
  // weld: sort the indices by (coordinate bits, index); a run of equal coordinates is one vertex, its first index the name
  std::vector<int> weld((size_t)Nv), order((size_t)Nv);
  for (int i = 0; i < Nv; ++i) order[i] = i;
  auto bits = [&](int i, int k) { return ordered_bits(pos[(size_t)i * 3 + k]); };
  std::sort(order.begin(), order.end(), [&](int i, int j) {
    for (int k = 0; k < 3; ++k)
      if (bits(i, k) != bits(j, k)) return bits(i, k) < bits(j, k);
    return i < j;
  });
  int welded = 0;
  for (int r = 0, head = 0; r < Nv; ++r) {
    const int i = order[r];
    const float* x = pos + (size_t)i * 3;
    const bool nan = x[0] != x[0] || x[1] != x[1] || x[2] != x[2];
    const bool same = r > 0 && !nan && bits(i, 0) == bits(head, 0) && bits(i, 1) == bits(head, 1) && bits(i, 2) == bits(head, 2);
    if (!same) head = i;
    weld[i] = head;
    welded += same ? 1 : 0;
  }
  // per face: the unit normal (float64), the three angles into the welded vertices' sums, the three edge uses
  std::vector<double> acc((size_t)Nv * 3, 0.0), unit((size_t)F * 3, 0.0);
  std::vector<unsigned char> good((size_t)F, 0);
  std::vector<EdgeUse> uses;
  uses.reserve((size_t)F * 3);
  int degenerate = 0;
  for (int f = 0; f < F; ++f) {
    const int32_t* idx = faces + (size_t)f * 3;
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && (unsigned)idx[k] < (unsigned)Nv;
    double len = 0.0, n[3] = {0, 0, 0}, v[3][3] = {};
    if (ok) {
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) v[j][k] = (double)pos[(size_t)idx[j] * 3 + k];
      const double ab[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
      const double ac[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
      n[0] = ab[1] * ac[2] - ab[2] * ac[1];
      n[1] = ab[2] * ac[0] - ab[0] * ac[2];
      n[2] = ab[0] * ac[1] - ab[1] * ac[0];
      len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    }
    if (!(ok && len > 0.0 && len <= 1.79769313486231570815e308)) {   // zero area, a NaN or an overflow: no normal
      ++degenerate;
      continue;
    }
    good[f] = 1;
    for (int k = 0; k < 3; ++k) unit[(size_t)f * 3 + k] = n[k] / len;
    for (int j = 0; j < 3; ++j) {   // corner j: the angle between the edges to the next and to the previous corner
      const double* o = v[j];
      const double* x = v[(j + 1) % 3];
      const double* y = v[(j + 2) % 3];
      const double e0[3] = {x[0] - o[0], x[1] - o[1], x[2] - o[2]}, e1[3] = {y[0] - o[0], y[1] - o[1], y[2] - o[2]};
      const double d = (e0[0] * e1[0] + e0[1] * e1[1]) + e0[2] * e1[2];
      const double l0 = sqrt((e0[0] * e0[0] + e0[1] * e0[1]) + e0[2] * e0[2]), l1 = sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
      double c = d / (l0 * l1);
      c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;
      const double angle = acos(c);
      const int w = weld[idx[j]];
      for (int k = 0; k < 3; ++k) acc[(size_t)w * 3 + k] += angle * unit[(size_t)f * 3 + k];
      const int w0 = w, w1 = weld[idx[(j + 1) % 3]];   // edge j: ab, bc, ca
      const bool fwd = w0 < w1;
      uses.push_back(EdgeUse{((unsigned long long)(unsigned)(fwd ? w0 : w1) << 32) | (unsigned)(fwd ? w1 : w0), f, fwd});
    }
  }
  std::sort(uses.begin(), uses.end(), [](const EdgeUse& a, const EdgeUse& b) { return a.key != b.key ? a.key < b.key : a.face < b.face; });
  // runs of one key: the edge's faces in index order
  int edges = 0, boundary = 0, nonmanifold = 0, inconsistent = 0;
  std::vector<unsigned long long> keys;
  std::vector<double> sums;
  for (size_t r = 0; r < uses.size();) {
    size_t e = r;
    double s[3] = {0, 0, 0};
    for (; e < uses.size() && uses[e].key == uses[r].key; ++e)
      for (int k = 0; k < 3; ++k) s[k] += unit[(size_t)uses[e].face * 3 + k];
    const size_t cnt = e - r;
    ++edges;
    boundary += cnt == 1;
    nonmanifold += cnt > 2;
    inconsistent += cnt == 2 && uses[r].forward == uses[r + 1].forward;
    keys.push_back(uses[r].key);
    sums.insert(sums.end(), s, s + 3);
    r = e;
  }
  for (int i = 0; i < Nv; ++i)
    for (int k = 0; k < 3; ++k) vn[(size_t)i * 3 + k] = (float)acc[(size_t)weld[i] * 3 + k];
  for (int f = 0; f < F; ++f) {
    const int32_t* idx = faces + (size_t)f * 3;
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && (unsigned)idx[k] < (unsigned)Nv;
    for (int j = 0; j < 3; ++j) {
      double s[3] = {0, 0, 0};
      if (ok) {   // a degenerate face's edge carries the normals of the faces that share it, like any other
        const int w0 = weld[idx[j]], w1 = weld[idx[(j + 1) % 3]];
        const unsigned long long key = ((unsigned long long)(unsigned)std::min(w0, w1) << 32) | (unsigned)std::max(w0, w1);
        const auto it = std::lower_bound(keys.begin(), keys.end(), key);
        if (it != keys.end() && *it == key)
          for (int k = 0; k < 3; ++k) s[k] = sums[(size_t)(it - keys.begin()) * 3 + k];
      }
      for (int k = 0; k < 3; ++k) en[((size_t)f * 3 + j) * 3 + k] = (float)s[k];
    }
  }
  report[0] = edges;
  report[1] = boundary;
  report[2] = nonmanifold;
  report[3] = inconsistent;
  report[4] = degenerate;
  report[5] = welded;
  report[6] = edges > 0 && boundary == 0 && nonmanifold == 0 && inconsistent == 0;
  report[7] = 0;
  return FP_OK;
}
