// fsim_normals.hpp -- surface-normal and shaded images from the cameras (include/fsim_normals.h).  Included at the end of fsim.hip,
// after fsim_voxels.hpp: the host part renders through cam_render_images (fsim_render: k_cam_pose, k_cam_ray, as they are); the kernel
// stages the geom poses k_cam_pose leaves in the handle's pose scratch as k_cam_ray does and the camera poses with
// cam_stage_views, and back-projects through pts_point, the function k_pts_gather and k_vox_bin call.
//
// After fsim_render's two launches, on the same stream:
//   k_cam_normal  one 256-thread workgroup per (env, camera, chunk of up to NRM_CHUNK pixels).  The env's geom table (pose + static
//                 words, k_cam_ray's layout), the hull planes, the camera poses and the model-geom-id -> colliding-geom table are staged
//                 in LDS once; then every lane takes one pixel per round from coalesced reads of depth and seg, brings its world point
//                 into the frame of the geom it sees and evaluates that geom's closed-form normal (only a pixel on a hull walks the
//                 hull's planes).  The shaded pixel is one dword store per lane, the normal three (12-byte stride between lanes: a
//                 wave's three stores cover the same 768 contiguous bytes).  Staging a round's normals in LDS to write them as fully
//                 coalesced dwords was measured and dropped: it was 11-25 % slower (profiles/nrm_a_store_comparison.txt).
// No atomics, no scratch: every pixel is written once, and an env's output depends on nothing but its images, its poses and the settings.
#include "../../include/fsim_normals.h"

#define NRM_THREADS 256 // k_cam_normal
#define NRM_CHUNK 2048  // pixels per workgroup: eight rounds share one staging of the tables
#define NRM_TINY 1e-20f // a shorter vector has no direction: (0, 0, 0)
#define NRM_NOGEOM 0xff // id table: a model geom that does not collide (never seen by a camera)

struct NrmArgs {
  CamView v;
  int hw /* W * H */, ngeom, nplanes, nchunk;
  float ambient;
  unsigned background; // RGBA, R in the low byte
};

DEV V3 nrm_unit(V3 a) { // a / |a|, (0, 0, 0) for a degenerate length
  const float l = norm(a);
  return l < NRM_TINY ? v3(0.0f, 0.0f, 0.0f) : a * (1.0f / l);
}

// the header's local outward normal at the point p of the geom row G (k_cam_ray's staged layout); PL: the staged hull planes
DEV V3 nrm_local(const float *G, const float *PL, V3 p) {
  const int type = __float_as_int(G[CGW_TYPE]);
  const float s0 = G[CGW_SIZE], s1 = G[CGW_SIZE + 1], s2 = G[CGW_SIZE + 2];
  if (type == GT_PLANE) return v3(0.0f, 0.0f, 1.0f);
  if (type == GT_SPHERE) return nrm_unit(p);
  if (type == GT_CAPSULE) return nrm_unit(v3(p.x, p.y, p.z - fminf(fmaxf(p.z, -s1), s1)));
  if (type == GT_CYLINDER) {
    const float rho = sqrtf(p.x * p.x + p.y * p.y);
    if (rho - s0 >= fabsf(p.z) - s1) return rho < NRM_TINY ? v3(0.0f, 0.0f, 0.0f) : v3(p.x, p.y, 0.0f) * (1.0f / rho); // the side wins a tie
    return v3(0.0f, 0.0f, p.z < 0.0f ? -1.0f : 1.0f);
  }
  if (type == GT_BOX) { // strict >: the smallest axis wins a tie
    const float ex = fabsf(p.x) - s0, ey = fabsf(p.y) - s1, ez = fabsf(p.z) - s2;
    int a = 0;
    float best = ex;
    if (ey > best) { best = ey; a = 1; }
    if (ez > best) a = 2;
    const float sg = comp(p, a) < 0.0f ? -1.0f : 1.0f;
    return v3(a == 0 ? sg : 0.0f, a == 1 ? sg : 0.0f, a == 2 ? sg : 0.0f);
  }
  if (type == GT_MESH) { // strict >: the smallest k wins a tie
    const int p0 = __float_as_int(G[CGW_PADR]), np = __float_as_int(G[CGW_PNUM]);
    V3 n = v3(0.0f, 0.0f, 0.0f);
    float best = -CAM_INF;
    for (int k = 0; k < np; k++) {
      const float *pl = PL + 4 * (p0 + k);
      const V3 nk = ldv3(pl);
      const float v = dot(nk, p) - pl[3];
      if (v > best) { best = v; n = nk; }
    }
    return n;
  }
  return v3(0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(NRM_THREADS) void k_cam_normal(NrmArgs a, const float *__restrict__ pose, const float *__restrict__ cgtab,
                                                            const float *__restrict__ planes_g, const unsigned char *__restrict__ idtab_g,
                                                            const unsigned *__restrict__ palette, const float *__restrict__ depth,
                                                            const int *__restrict__ seg, float *__restrict__ normal, unsigned *__restrict__ shaded) {
  extern __shared__ float nrm_lds[];
  float *G = nrm_lds;                      // [ncg][CAM_GW]
  float *PL = G + CAM_GW * a.v.ncg;        // [nplanes][4]
  float *cpose = PL + 4 * a.nplanes;       // [FSIM_CAM_MAX][CAM_PW]
  float *cslope = cpose + FSIM_CAM_MAX * CAM_PW; // [FSIM_CAM_MAX]
  unsigned char *idtab = reinterpret_cast<unsigned char *>(cslope + FSIM_CAM_MAX); // [ngeom]
  int blk = blockIdx.x;
  const int chunk = blk % a.nchunk; blk /= a.nchunk;
  const int cam = blk % a.v.ncam, e = blk / a.v.ncam, tid = threadIdx.x;
  const float *P = pose + (size_t)e * a.v.pstride;
  for (int i = tid; i < CAM_PW * a.v.ncg; i += NRM_THREADS) G[CAM_GW * (i / CAM_PW) + i % CAM_PW] = P[i]; // (k_cam_ray's three loops)
  for (int i = tid; i < CAM_SW * a.v.ncg; i += NRM_THREADS) G[CAM_GW * (i / CAM_SW) + CAM_PW + i % CAM_SW] = cgtab[i];
  for (int i = tid; i < 4 * a.nplanes; i += NRM_THREADS) PL[i] = planes_g[i];
  cam_stage_views(cpose, cslope, P + CAM_PW * a.v.ncg, a.v, tid, NRM_THREADS);
  for (int i = tid; i < a.ngeom; i += NRM_THREADS) idtab[i] = idtab_g[i];
  __syncthreads();
  const V3 co = ldv3(cpose + CAM_PW * cam);
  const int c0 = chunk * NRM_CHUNK, len = min(NRM_CHUNK, a.hw - c0); // this workgroup's pixels of the (env, camera) image
  const size_t img = (size_t)e * a.v.npix + (size_t)cam * a.hw + c0;    // the first of them, in pixels of the whole batch
  for (int r0 = 0; r0 < len; r0 += NRM_THREADS) {
    const int r = r0 + tid;
    V3 n = v3(0.0f, 0.0f, 0.0f);
    if (r < len) {
      const int g = seg[img + r];
      unsigned px = a.background;
      if (g >= 0 && g < a.ngeom) {
        const V3 q = pts_point(cpose, cslope, a.v.W, a.v.H, cam * a.hw + c0 + r, depth[img + r]);
        const int ci = idtab[g];
        if (ci != NRM_NOGEOM) { // (always: the ray pass names colliding geoms only; otherwise the normal stays (0, 0, 0))
          const float *Gg = G + CAM_GW * ci;
          const M3 Rg = ldm3(Gg + CGW_MAT);
          n = mulv(Rg, nrm_local(Gg, PL, multv(Rg, q - ldv3(Gg + CGW_POS))));
        }
        if (shaded) {
          const float lam = fabsf(dot(n, nrm_unit(co - q)));
          const float I = a.ambient + (1.0f - a.ambient) * lam;
          const unsigned c = palette[g];
          const unsigned cr = (unsigned)fminf(floorf((float)(c & 0xffu) * I + 0.5f), 255.0f);
          const unsigned cg = (unsigned)fminf(floorf((float)((c >> 8) & 0xffu) * I + 0.5f), 255.0f);
          const unsigned cb = (unsigned)fminf(floorf((float)((c >> 16) & 0xffu) * I + 0.5f), 255.0f);
          px = cr | (cg << 8) | (cb << 16) | (c & 0xff000000u);
        }
      }
      if (shaded) shaded[img + r] = px;
    }
    if (normal && r < len) stv3(normal + 3 * (img + r), n); // (a wave's 64 pixels: 768 contiguous bytes over three dword stores)
  }
}

// ------------------------------------------------------------------------------------------ host
struct NrmState {
  bool has_palette = false;
  float ambient = 0.0f;
  unsigned background = 0u;
  unsigned *d_palette = nullptr;                  // [ngeom] RGBA, R in the low byte
  unsigned char *d_idtab = nullptr;               // [ngeom] model geom id -> colliding geom (row of the staged table), NRM_NOGEOM: none
};

static void nrm_free(fsim *s) {
  if (!s->nrm) return;
  hipFree(s->nrm->d_palette); hipFree(s->nrm->d_idtab);
  delete s->nrm;
  s->nrm = nullptr;
}

// The model-geom-id -> colliding-geom table [max(ngeom, 1)] k_cam_normal and k_cam_flow (fsim_flow.hpp) stage: the row of the staged geom
// table that shows model geom g, NRM_NOGEOM for a geom that does not collide.
static int nrm_idtab(const fsim *s, std::vector<unsigned char> &idtab) {
  std::vector<int> cg_orig;
  if (!blob_i(s->blob, "cg_orig", cg_orig)) return FSIM_EINVAL;
  idtab.assign(std::max(s->ngeom, 1), NRM_NOGEOM);
  for (int k = 0; k < s->m.ncg; k++)
    if (cg_orig[k] >= 0 && cg_orig[k] < s->ngeom) idtab[cg_orig[k]] = (unsigned char)k;
  return FSIM_OK;
}

extern "C" int fsim_set_normals(fsim_t *s, const uint8_t *palette, const uint8_t background[4], float ambient) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_normals: null handle");
  if (!std::isfinite(ambient) || ambient < 0.0f || ambient > 1.0f) FAIL(FSIM_EINVAL, "fsim_set_normals: ambient %g (0 .. 1)", ambient);
  if (s->m.ncg > FSIM_CAM_MAX_GEOMS) FAIL(FSIM_EINVAL, "fsim_set_normals: %d colliding geoms (the cameras stage at most %d)", s->m.ncg, FSIM_CAM_MAX_GEOMS);
  const int ng = std::max(s->ngeom, 1);
  std::vector<unsigned char> idtab;
  { int rc_ = nrm_idtab(s, idtab); if (rc_) return rc_; }
  std::vector<unsigned> pal(ng, 0u);
  if (palette)
    for (int g = 0; g < s->ngeom; g++)
      pal[g] = (unsigned)palette[4 * g] | ((unsigned)palette[4 * g + 1] << 8) | ((unsigned)palette[4 * g + 2] << 16) | ((unsigned)palette[4 * g + 3] << 24);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream)); // (a render in flight still reads the old tables)
  if (!s->nrm) {
    s->nrm = new NrmState();
    HIPCHK(hipMalloc(&s->nrm->d_palette, (size_t)ng * 4));
    HIPCHK(hipMalloc(&s->nrm->d_idtab, ng));
  }
  NrmState &v = *s->nrm;
  v.has_palette = palette != nullptr;
  v.ambient = ambient;
  v.background = background ? (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16) | ((unsigned)background[3] << 24) : 0u;
  HIPCHK(hipMemcpy(v.d_palette, pal.data(), (size_t)ng * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v.d_idtab, idtab.data(), ng, hipMemcpyHostToDevice));
  return FSIM_OK;
}

extern "C" int fsim_render_normals(fsim_t *s, float *depth_dev, int32_t *seg_dev, float *normal_dev, uint8_t *shaded_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_render_normals: null handle");
  if (!s->cam) FAIL(FSIM_EINVAL, "fsim_render_normals: no cameras set (fsim_set_cameras)");
  if (!s->nrm) FAIL(FSIM_EINVAL, "fsim_render_normals: no normals settings (fsim_set_normals)");
  if (!normal_dev && !shaded_dev) FAIL(FSIM_EINVAL, "fsim_render_normals: no output (normal and shaded both NULL)");
  NrmState &v = *s->nrm;
  const CamState &k = *s->cam;
  if (shaded_dev && !v.has_palette) FAIL(FSIM_EINVAL, "fsim_render_normals: shaded_dev given without a palette (fsim_set_normals)");
  if (reinterpret_cast<uintptr_t>(shaded_dev) & 3) FAIL(FSIM_EINVAL, "fsim_render_normals: shaded_dev is not 4-byte aligned");
  const int hw = k.W * k.H;
  const int nchunk = (hw + NRM_CHUNK - 1) / NRM_CHUNK;
  const size_t nblk = (size_t)s->n_envs * k.ncam * nchunk;
  if (nblk > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_render_normals: %zu workgroups", nblk);
  const size_t lds = 4 * ((size_t)CAM_GW * s->m.ncg + 4 * k.nplanes + FSIM_CAM_MAX * CAM_PW + FSIM_CAM_MAX) + (size_t)s->ngeom;
  if (lds > 65536) FAIL(FSIM_EINVAL, "fsim_render_normals: %d geoms need %zu bytes of LDS (at most 65536)", s->ngeom, lds);
  HIPCHK(hipSetDevice(s->device));
  const float *depth;
  const int *seg;
  { int rc_ = cam_render_images(s, depth_dev, seg_dev, &depth, &seg); if (rc_) return rc_; }
  NrmArgs na{};
  na.v = cam_view(s); na.hw = hw; na.ngeom = s->ngeom; na.nplanes = k.nplanes; na.nchunk = nchunk; na.ambient = v.ambient; na.background = v.background;
  hipLaunchKernelGGL(k_cam_normal, dim3((unsigned)nblk), dim3(NRM_THREADS), lds, s->stream, na, k.d_pose, k.d_cg, k.d_planes, v.d_idtab, v.d_palette,
                     depth, seg, normal_dev, reinterpret_cast<unsigned *>(shaded_dev));
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
