// test tool (tests/test_pairs_tool_gpu.py; built into tests/libpair_distance_probe.so with the library's own floating-point flags): the per-pair
// routine of furniture_amd/csrc/fsim_gjk.hpp (gjk_pair: plane closed form, GJK on the cores, hand-off to np_mpr), called on arbitrary shapes
// -- one lane per case, no model, no LDS.  The routine is the library's template, included as it is; nothing here restates it.
//
// case record: the 36 floats and 3 ints of tests/narrowphase_probe.hip (p1[3] R1[9] s1[3] p2[3] R2[9] s2[3] ... | pair type, geom type 1, geom type 2)
// result record, 12 floats: d, normal[3], from[3], to[3], GJK iterations, branch (GJK_BR_*)
#include "../furniture_amd/csrc/fsim_gjk.hpp"

#define PD_CASEW 36
#define PD_OUTW 12

__global__ __launch_bounds__(64) void k_pd_pairs(const float *cases, const int *types, int n, const float *verts, int nvert, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *c = cases + PD_CASEW * (size_t)i;
  const MeshVerts mv = (MeshVerts)verts;
  Shape A, B;
  A.type = types[3 * i + 1]; A.pos = ldv3(c); A.R = ldm3(c + 3); A.size = ldv3(c + 12);
  B.type = types[3 * i + 2]; B.pos = ldv3(c + 15); B.R = ldm3(c + 18); B.size = ldv3(c + 27);
  A.verts = mv; A.nvert = A.type == GT_MESH ? nvert : 0; B.verts = mv; B.nvert = B.type == GT_MESH ? nvert : 0;
  const PairOut o = gjk_pair<true>(A, B);
  float *r = out + PD_OUTW * (size_t)i;
  r[0] = o.d;
  stv3(r + 1, o.n); stv3(r + 4, o.from); stv3(r + 7, o.to);
  r[10] = (float)o.iters; r[11] = (float)o.branch;
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
};
} // namespace
#define PD_CK(x) do { hipError_t rc_ = (x); if (rc_ != hipSuccess) return (int)rc_; } while (0)

// host entry: host pointers in, host pointer out; 0 or the HIP error code
extern "C" int pd_probe_pairs(const float *cases, const int *types, int n, const float *verts, int nvert, float *out) {
  if (n <= 0) return 0;
  DevBuf dc(sizeof(float) * PD_CASEW * n, cases), dt(sizeof(int) * 3 * n, types), dv(sizeof(float) * 3 * nvert, verts), dout(sizeof(float) * PD_OUTW * n, nullptr);
  PD_CK(dc.rc); PD_CK(dt.rc); PD_CK(dv.rc); PD_CK(dout.rc);
  hipLaunchKernelGGL(k_pd_pairs, dim3((n + 63) / 64), dim3(64), 0, 0, (const float *)dc.p, (const int *)dt.p, n, (const float *)dv.p, nvert, (float *)dout.p);
  PD_CK(hipGetLastError());
  PD_CK(hipDeviceSynchronize());
  PD_CK(hipMemcpy(out, dout.p, sizeof(float) * PD_OUTW * n, hipMemcpyDeviceToHost));
  return 0;
}
