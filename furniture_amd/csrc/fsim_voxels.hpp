// fsim_voxels.hpp -- voxel-grid observations binned from the cameras (include/fsim_voxels.h).  Included at the end of fsim.hip, after
// fsim_points.hpp: the host part renders through cam_render_images (fsim_render: k_cam_pose, k_cam_ray, as they are); the kernel stages
// the camera poses with cam_stage_views, back-projects through pts_point and keeps a pixel by pts_seg_kept and pts_in_box, the
// functions k_pts_gather calls.
//
// After fsim_render's two launches, on the same stream:
//   k_vox_bin  one 1024-thread workgroup per (env, chunk of up to VOX_CHUNK cells).  The chunk's cells live in LDS as a 32-bit count and
//              a 32-bit smallest pix each (8 B per cell, 128 KB for a full chunk).  The workgroup walks every pixel of the env,
//              back-projects the kept ones, computes their cell and, for the cells of its chunk, adds 1 to the count and takes the min
//              of pix with LDS atomics.  After one barrier it writes the chunk out as int16: count (saturated) and label = seg at the
//              smallest pix, 8 cells per 128-bit store when the layout allows it.
// Integer add and min do not depend on the order of arrival: the grid is bit-reproducible whatever the schedule.  No global atomics; an
// env's grid depends on nothing but its images, its camera poses and the settings.
#include "../../include/fsim_voxels.h"

#define VOX_THREADS 1024  // k_vox_bin
#define VOX_CHUNK 16384   // cells per workgroup: 128 KB of LDS, within the 160 KiB of a gfx950 CU
#define VOX_EMPTY 0x7fffffffu // smallest pix of a cell no pixel has reached

struct VoxArgs {
  CamView v;
  int dx, dy, dz, ncells, nchunk, vec /* 128-bit stores: ncells % 8 == 0 and both outputs 16-B aligned */;
  float lo[3], hi[3], sc[3]; // the box and s_a = dims_a / (hi_a - lo_a), rounded once on the host
};

// the header's cell index along one axis: t = (p - lo) * s with every operation rounded on its own (hipcc contracts by default), then
// floor, clamped to the last cell (p == hi)
DEV int vox_axis(float p, float lo, float s, int n) {
#pragma clang fp contract(off)
  const float t = (p - lo) * s;
  return min((int)floorf(t), n - 1);
}

DEV unsigned vox_pack(int lo16, int hi16) { return ((unsigned)lo16 & 0xffffu) | ((unsigned)hi16 << 16); }

__global__ __launch_bounds__(VOX_THREADS) void k_vox_bin(VoxArgs a, const float *__restrict__ pose, const float *__restrict__ depth,
                                                         const int *__restrict__ seg, const unsigned char *__restrict__ keep,
                                                         short *__restrict__ count, short *__restrict__ label) {
  extern __shared__ unsigned vox_lds[]; // [0, len) counts, [len, 2 len) smallest pix of the chunk's cells
  __shared__ float cpose[FSIM_CAM_MAX * CAM_PW], cslope[FSIM_CAM_MAX];
  const int e = blockIdx.x / a.nchunk, chunk = blockIdx.x - e * a.nchunk, tid = threadIdx.x;
  const int c0 = chunk * VOX_CHUNK, len = min(VOX_CHUNK, a.ncells - c0);
  unsigned *cnt = vox_lds, *mp = vox_lds + len;
  cam_stage_views(cpose, cslope, pose + (size_t)e * a.v.pstride + CAM_PW * a.v.ncg, a.v, tid, VOX_THREADS);
  for (int i = tid; i < len; i += VOX_THREADS) {
    cnt[i] = 0u;
    mp[i] = VOX_EMPTY;
  }
  __syncthreads();
  const size_t base = (size_t)e * a.v.npix;
  for (int p = tid; p < a.v.npix; p += VOX_THREADS) {
    if (!pts_seg_kept(seg[base + p], keep)) continue;
    const V3 q = pts_point(cpose, cslope, a.v.W, a.v.H, p, depth[base + p]);
    if (!pts_in_box(q, a.lo, a.hi)) continue;
    const int c = (vox_axis(q.x, a.lo[0], a.sc[0], a.dx) * a.dy + vox_axis(q.y, a.lo[1], a.sc[1], a.dy)) * a.dz +
                  vox_axis(q.z, a.lo[2], a.sc[2], a.dz) - c0;
    if ((unsigned)c < (unsigned)len) {
      atomicAdd(cnt + c, 1u);
      atomicMin(mp + c, (unsigned)p);
    }
  }
  __syncthreads();
  const size_t o = (size_t)e * a.ncells + c0;
  if (a.vec) { // len % 8 == 0 and (o * 2 B) % 16 == 0: one 16-B store of counts and one of labels per 8 cells
    for (int i = 8 * tid; i < len; i += 8 * VOX_THREADS) {
      int cv[8], lv[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const unsigned n = cnt[i + j];
        cv[j] = (int)min(n, 32767u);
        lv[j] = n ? seg[base + mp[i + j]] : -1;
      }
      uint4 wc, wl;
      wc.x = vox_pack(cv[0], cv[1]); wc.y = vox_pack(cv[2], cv[3]); wc.z = vox_pack(cv[4], cv[5]); wc.w = vox_pack(cv[6], cv[7]);
      wl.x = vox_pack(lv[0], lv[1]); wl.y = vox_pack(lv[2], lv[3]); wl.z = vox_pack(lv[4], lv[5]); wl.w = vox_pack(lv[6], lv[7]);
      *reinterpret_cast<uint4 *>(count + o + i) = wc;
      *reinterpret_cast<uint4 *>(label + o + i) = wl;
    }
  } else {
    for (int i = tid; i < len; i += VOX_THREADS) {
      const unsigned n = cnt[i];
      count[o + i] = (short)min(n, 32767u);
      label[o + i] = (short)(n ? seg[base + mp[i]] : -1);
    }
  }
}

// ------------------------------------------------------------------------------------------ host
struct VoxState {
  int dims[3] = {0, 0, 0}, ncells = 0;
  float lo[3], hi[3], sc[3];
  unsigned char *d_keep = nullptr; // [ngeom]
};

static void vox_free(fsim *s) {
  if (!s->vox) return;
  hipFree(s->vox->d_keep);
  delete s->vox;
  s->vox = nullptr;
}

extern "C" int fsim_set_voxels(fsim_t *s, const int32_t dims[3], const float box[6], const uint8_t *geom_keep) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_voxels: null handle");
  if (s->ngeom > 32767) FAIL(FSIM_EINVAL, "fsim_set_voxels: the model has %d geoms (labels are int16: at most 32767)", s->ngeom);
  if (!dims || !box) FAIL(FSIM_EINVAL, "fsim_set_voxels: a NULL dims or box (the box is required)");
  long cells = 1;
  for (int i = 0; i < 3; i++) {
    if (dims[i] < 1 || dims[i] > FSIM_VOX_MAX_DIM) FAIL(FSIM_EINVAL, "fsim_set_voxels: dims[%d] = %d (1 .. %d)", i, dims[i], FSIM_VOX_MAX_DIM);
    cells *= dims[i];
  }
  if (cells > FSIM_VOX_MAX_CELLS) FAIL(FSIM_EINVAL, "fsim_set_voxels: %d x %d x %d = %ld cells (at most %d)", dims[0], dims[1], dims[2], cells, FSIM_VOX_MAX_CELLS);
  if (pts_box_finite("fsim_set_voxels", box)) return FSIM_EINVAL;
  float sc[3];
  for (int i = 0; i < 3; i++) {
    if (!(box[i] < box[3 + i])) FAIL(FSIM_EINVAL, "fsim_set_voxels: box lo %g >= hi %g on axis %d", box[i], box[3 + i], i);
    const float ext = box[3 + i] - box[i];
    sc[i] = (float)dims[i] / ext; // the header's s_a: IEEE fp32 division on the host
    if (!std::isfinite(ext) || !std::isnormal(sc[i]))
      FAIL(FSIM_EINVAL, "fsim_set_voxels: box extent %g on axis %d gives the scale %g (not a finite normal fp32)", ext, i, sc[i]);
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream)); // (a render in flight still reads the old keep table)
  if (!s->vox) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_vox_bin), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * VOX_CHUNK));
    s->vox = new VoxState();
  }
  VoxState &v = *s->vox;
  for (int i = 0; i < 3; i++) {
    v.dims[i] = dims[i];
    v.lo[i] = box[i];
    v.hi[i] = box[3 + i];
    v.sc[i] = sc[i];
  }
  v.ncells = (int)cells;
  return pts_upload_keep(s, geom_keep, &v.d_keep);
}

extern "C" int fsim_render_voxels(fsim_t *s, float *depth_dev, int32_t *seg_dev, int16_t *count_dev, int16_t *label_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_render_voxels: null handle");
  if (!s->vox) FAIL(FSIM_EINVAL, "fsim_render_voxels: no voxel settings (fsim_set_voxels)");
  if (!s->cam) FAIL(FSIM_EINVAL, "fsim_render_voxels: no cameras set (fsim_set_cameras)");
  if (!count_dev || !label_dev) FAIL(FSIM_EINVAL, "fsim_render_voxels: a NULL output");
  VoxState &v = *s->vox;
  const CamState &k = *s->cam;
  const int nchunk = (v.ncells + VOX_CHUNK - 1) / VOX_CHUNK;
  const size_t nblk = (size_t)s->n_envs * nchunk;
  if (nblk > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_render_voxels: %zu workgroups", nblk);
  HIPCHK(hipSetDevice(s->device));
  const float *depth;
  const int *seg;
  { int rc_ = cam_render_images(s, depth_dev, seg_dev, &depth, &seg); if (rc_) return rc_; }
  VoxArgs va{};
  va.v = cam_view(s);
  va.dx = v.dims[0]; va.dy = v.dims[1]; va.dz = v.dims[2]; va.ncells = v.ncells; va.nchunk = nchunk;
  va.vec = v.ncells % 8 == 0 && (reinterpret_cast<uintptr_t>(count_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(label_dev) & 15) == 0;
  for (int i = 0; i < 3; i++) { va.lo[i] = v.lo[i]; va.hi[i] = v.hi[i]; va.sc[i] = v.sc[i]; }
  const size_t lds = 8 * (size_t)std::min(v.ncells, VOX_CHUNK);
  hipLaunchKernelGGL(k_vox_bin, dim3((unsigned)nblk), dim3(VOX_THREADS), lds, s->stream, va, k.d_pose, depth, seg, v.d_keep, count_dev, label_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
