// test tool (tests/test_narrowphase_gpu.py; built into tests/libnarrowphase_probe.so with the library's own floating-point flags): the narrow-phase
// routines of furniture_amd/csrc/fsim_collide.hpp, called pair by pair with a recording emitter -- one lane per case, no model, no LDS.
// The routines are the library's templates, included as they are; nothing here restates them.
//
// case record, 36 floats: p1[3] R1[9] s1[3] p2[3] R2[9] s2[3] margin rbound1 rbound2 | 3 ints: pair type (PT_*), geom type 1, geom type 2
// contact record, 8 floats: active, dist, pos[3], unit normal[3]; at most NP_MAXC per case
#include "../furniture_amd/csrc/fsim_collide.hpp"

#define NP_MAXC 16
#define NP_CASEW 36
#define NP_CONW 8

// what Emit does with a contact, minus the LDS slot and the solver parameters: the same count limit, the same finite / degenerate filter
struct Rec {
  float *out;  // NP_MAXC contact records of this case
  int *cnt;
  int maxn;
  float margin;
  DEV void put(int slot, bool ok, float dist, V3 pos, V3 n) const {
    float *r = out + NP_CONW * slot;
    r[0] = ok ? 1.0f : 0.0f;
    r[1] = dist;
    stv3(r + 2, pos);
    stv3(r + 5, ok ? normalized(n) : n);
  }
  DEV void operator()(int k, float dist, V3 pos, V3 n) const {
    if (k >= maxn) return;
    if (!(isfinite(dist) && isfinite(pos.x + pos.y + pos.z) && isfinite(n.x + n.y + n.z)) || dot(n, n) < 1e-12f) return;
    const int slot = (*cnt)++;
    if (slot >= NP_MAXC) return;
    put(slot, true, dist, pos, n);
  }
  DEV int alloc(int &n) const {
    const int base = *cnt;
    *cnt += n;
    if (base + n > NP_MAXC) n = max(0, NP_MAXC - base);
    return n > 0 ? base : -1;
  }
  DEV void write(int slot, float dist, V3 pos, V3 n) const {
    const bool ok = isfinite(dist) && isfinite(pos.x + pos.y + pos.z) && isfinite(n.x + n.y + n.z) && dot(n, n) >= 1e-12f;
    put(slot, ok, dist, pos, n); // (a degenerate result keeps its slot, inactive)
  }
};

struct Case { V3 p1, s1, p2, s2; M3 R1, R2; float margin, r1, r2; int pt, t1, t2; };
DEV Case np_load(const float *cases, const int *types, int i) {
  const float *c = cases + NP_CASEW * (size_t)i;
  Case k;
  k.p1 = ldv3(c); k.R1 = ldm3(c + 3); k.s1 = ldv3(c + 12); k.p2 = ldv3(c + 15); k.R2 = ldm3(c + 18); k.s2 = ldv3(c + 27);
  k.margin = c[30]; k.r1 = c[31]; k.r2 = c[32];
  k.pt = types[3 * i]; k.t1 = types[3 * i + 1]; k.t2 = types[3 * i + 2];
  return k;
}

// the pair-type dispatch of fs_collide, without its pre-tests
// MESH: the np_mpr the generic kernels run (hull support compiled in) / the one of the kernels specialised for one model (the benchmark's)
template <bool MESH> __global__ void k_np_contacts(const float *cases, const int *types, int n, const float *verts, int nvert, float *out, int *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Case k = np_load(cases, types, i);
  if (k.pt < 0 || k.pt > PT_PLANE_MESH) { count[i] = -1; return; }
  int cnt = 0;
  Rec e;
  e.out = out + (size_t)NP_MAXC * NP_CONW * i; e.cnt = &cnt; e.maxn = FS_PAIR_MAXCON[k.pt]; e.margin = k.margin;
  const MeshVerts mv = (MeshVerts)verts;
  const V3 p1 = k.p1, p2 = k.p2, s1 = k.s1, s2 = k.s2;
  const M3 R1 = k.R1, R2 = k.R2;
  switch (k.pt) {
    case PT_PLANE_SPHERE: np_plane_sphere(e, p1, R1, p2, s2.x); break;
    case PT_PLANE_BOX: np_plane_box(e, p1, R1, p2, R2, s2); break;
    case PT_PLANE_CYL: np_plane_cylinder(e, p1, R1, p2, R2, s2); break;
    case PT_SPHERE_SPHERE: np_sphere_sphere(e, p1, s1.x, p2, s2.x); break;
    case PT_SPHERE_BOX: np_sphere_box(e, p1, s1.x, p2, R2, s2); break;
    case PT_SPHERE_CYL: np_sphere_cylinder(e, p1, s1.x, p2, R2, s2); break;
    case PT_BOX_BOX: np_box_box(e, p1, R1, s1, p2, R2, s2); break;
    case PT_PLANE_CAP: {
      const V3 ax = colv(R2, 2);
      np_plane_sphere(e, p1, R1, p2 + ax * s2.y, s2.x);
      np_plane_sphere(e, p1, R1, p2 - ax * s2.y, s2.x);
      break;
    }
    case PT_PLANE_MESH: np_plane_mesh(e, p1, R1, p2, R2, mv, nvert); break;
    default: {
      Shape A, B;
      A.type = k.t1; A.pos = p1; A.R = R1; A.size = s1;
      B.type = k.t2; B.pos = p2; B.R = R2; B.size = s2;
      A.verts = mv; A.nvert = k.t1 == GT_MESH ? nvert : 0; B.verts = mv; B.nvert = k.t2 == GT_MESH ? nvert : 0;
      np_mpr<Rec, MESH>(e, A, B);
    }
  }
  count[i] = min(cnt, NP_MAXC);
}

// the early-outs of fs_collide.  verdict bits: 1 np_capsule_gap - r1 - r2 > margin, 2 np_cyl_cyl_separated (both PT_CYL_CYL), 4 np_cyl_box_separated
// (PT_CYL_BOX), 8 stage 2 of the broadphase (fs_stage2_near) says "cannot touch" (every pair type); capgap: np_capsule_gap - r1 - r2 (PT_CYL_CYL, else 0)
__global__ void k_np_pretests(const float *cases, const int *types, int n, int *verdict, float *capgap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Case k = np_load(cases, types, i);
  int v = 0;
  float g = 0.0f;
  if (k.pt == PT_CYL_CYL) {
    g = np_capsule_gap(k.p1, colv(k.R1, 2), k.s1.y, k.p2, colv(k.R2, 2), k.s2.y) - k.s1.x - k.s2.x;
    if (g > k.margin) v |= 1;
    if (np_cyl_cyl_separated(k.p1, colv(k.R1, 2), k.s1, k.p2, colv(k.R2, 2), k.s2, k.margin)) v |= 2;
  }
  if (k.pt == PT_CYL_BOX && np_cyl_box_separated(k.p1, k.R1, k.s1, k.p2, k.R2, k.s2, k.margin)) v |= 4;
  f4_t q2, q3;
  q2.x = k.s1.x; q2.y = k.s1.y; q2.z = k.s1.z; q2.w = 0.0f;
  q3.x = k.s2.x; q3.y = k.s2.y; q3.z = k.s2.z; q3.w = 0.0f;
  if (!fs_stage2_near(k.t1, k.t2, k.p2 - k.p1, k.R1, k.R2, q2, q3, k.margin, k.r1, k.r2)) v |= 8;
  verdict[i] = v;
  capgap[i] = g;
}

namespace {
struct DevBuf {
  void *p = nullptr;
  hipError_t rc = hipSuccess;
  DevBuf(size_t bytes, const void *src) {
    rc = hipMalloc(&p, bytes ? bytes : 4);
    if (rc == hipSuccess && src && bytes) rc = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    else if (rc == hipSuccess) rc = hipMemset(p, 0, bytes ? bytes : 4);
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t get(void *dst, size_t bytes) const { return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost); }
};
} // namespace
#define NP_CK(x) do { hipError_t rc_ = (x); if (rc_ != hipSuccess) return (int)rc_; } while (0)

// host entries: host pointers in, host pointers out; 0 or the HIP error code
// the device's FS_PAIR_MAXCON table (12 ints), so that the tests do not restate it
extern "C" int np_probe_maxcon(int *out12) { return (int)hipMemcpyFromSymbol(out12, HIP_SYMBOL(FS_PAIR_MAXCON), sizeof(int) * 12); }
extern "C" int np_probe_contacts(const float *cases, const int *types, int n, const float *verts, int nvert, float *out, int *count, int mesh) {
  if (n <= 0) return 0;
  DevBuf dc(sizeof(float) * NP_CASEW * n, cases), dt(sizeof(int) * 3 * n, types), dv(sizeof(float) * 3 * nvert, verts),
      dout(sizeof(float) * NP_MAXC * NP_CONW * n, nullptr), dcnt(sizeof(int) * n, nullptr);
  NP_CK(dc.rc); NP_CK(dt.rc); NP_CK(dv.rc); NP_CK(dout.rc); NP_CK(dcnt.rc);
  if (mesh) hipLaunchKernelGGL(k_np_contacts<true>, dim3((n + 63) / 64), dim3(64), 0, 0, (const float *)dc.p, (const int *)dt.p, n, (const float *)dv.p, nvert, (float *)dout.p, (int *)dcnt.p);
  else hipLaunchKernelGGL(k_np_contacts<false>, dim3((n + 63) / 64), dim3(64), 0, 0, (const float *)dc.p, (const int *)dt.p, n, (const float *)dv.p, nvert, (float *)dout.p, (int *)dcnt.p);
  NP_CK(hipGetLastError());
  NP_CK(hipDeviceSynchronize());
  NP_CK(dout.get(out, sizeof(float) * NP_MAXC * NP_CONW * n));
  NP_CK(dcnt.get(count, sizeof(int) * n));
  return 0;
}
extern "C" int np_probe_pretests(const float *cases, const int *types, int n, int *verdict, float *capgap) {
  if (n <= 0) return 0;
  DevBuf dc(sizeof(float) * NP_CASEW * n, cases), dt(sizeof(int) * 3 * n, types), dver(sizeof(int) * n, nullptr), dg(sizeof(float) * n, nullptr);
  NP_CK(dc.rc); NP_CK(dt.rc); NP_CK(dver.rc); NP_CK(dg.rc);
  hipLaunchKernelGGL(k_np_pretests, dim3((n + 63) / 64), dim3(64), 0, 0, (const float *)dc.p, (const int *)dt.p, n, (int *)dver.p, (float *)dg.p);
  NP_CK(hipGetLastError());
  NP_CK(hipDeviceSynchronize());
  NP_CK(dver.get(verdict, sizeof(int) * n));
  NP_CK(dg.get(capgap, sizeof(float) * n));
  return 0;
}
