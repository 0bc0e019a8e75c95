// Training labels from keypoint annotations on the device: generate_heatmaps / generate_pafs of
// coco_data_loader.py:208-268, the ignore-mask dilation of :340 and, for downscale > 1, the
// F.resize_images of the targets in compute_loss (train_coco_pose_estimation.py:56-60) in one pass.
//
// Every label value is a function of one pixel coordinate and the poses, so a downscaled output
// pixel evaluates the label only at its four bilinear taps (v0,u0) (v0,u1) (v1,u0) (v1,u1) and
// combines them with the f32 weights and operation order of F.resize_images (postproc.hip
// up_combine): no full-resolution map is ever written.
//
// Host (labels_pack, plain double operations): per (frame, joint) the visible joints (x, y) in
// person order; per (frame, limb) the limbs with both joints visible and not identical as
// (fx, fy, ux, uy, vx, vy, dist) in person order, u = d / sqrt(dx*dx + dy*dy), v = u rotated by
// pi/2 with the reference's cos(pi/2) = 6.1e-17; for downscale > 1 the align-corners axis taps.
// Device (make_labels<NT>): one workgroup of 64 threads per (frame, 64 consecutive output pixels),
// one thread per output pixel, channels looped; a channel's records are staged through LDS in
// chunks of kLabChunk people (every lane reads the same record: an LDS broadcast), so the number of
// people per frame is unbounded.  float64 in the reference's operation order, cast to f32 per tap.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kLabThreads = 64;
constexpr int kLabChunk = 8;   // people (records of one joint or limb) per LDS chunk
constexpr int kJointRec = 2;   // x, y
constexpr int kLimbRec = 7;    // fx, fy, ux, uy, vx, vy, dist
constexpr int kLabGroups = OP_N_JOINTS + OP_N_LIMBS;
constexpr int kDilate = 16;    // cv2.MORPH_DILATE with ones((16, 16)), anchor 8: sources d-8 .. d+7

struct LabelArgs {
  const double* rec;    // records, then (downscale > 1) the axis taps [oh + ow][3]: i0, i0+1 - u, u - i0
  const int32_t* idx;   // [n][kLabGroups][2]: first double of the group's records, record count
  const uint8_t* mask;  // (n, h, w), nonzero = ignored; or null
  int32_t h, w, oh, ow;
  int64_t axis_off;
  double sigma2, paf_width;
  float* pafs;   // (n, 38, oh, ow) or null
  float* heat;   // (n, 19, oh, ow) or null
  uint8_t* ign;  // (n, oh, ow) or null
};

// F.resize_images' four-tap sum (oracle/postproc.c:62-68); NT == 1: the tap itself
template <int NT>
__device__ __forceinline__ float lab_combine(const float* wt, const float* v) {
  if (NT == 1) return v[0];
  float s = __fadd_rn(__fmul_rn(wt[0], v[0]), __fmul_rn(wt[1], v[1]));
  s = __fadd_rn(s, __fmul_rn(wt[2], v[2]));
  return __fadd_rn(s, __fmul_rn(wt[3], v[3]));
}

__device__ __forceinline__ bool lab_dilated(const uint8_t* __restrict__ m, int h, int w, int y, int x) {
  const int y0 = max(y - kDilate / 2, 0), y1 = min(y + kDilate / 2 - 1, h - 1);
  const int x0 = max(x - kDilate / 2, 0), x1 = min(x + kDilate / 2 - 1, w - 1);
  bool any = false;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) any |= m[(int64_t)yy * w + xx] != 0;
  return any;
}

template <int NT>
__global__ __launch_bounds__(kLabThreads) void make_labels(LabelArgs a) {
  __shared__ double srec[kLabChunk * kLimbRec];
  const int tid = threadIdx.x, f = blockIdx.y;
  const int plane = a.oh * a.ow;
  const int pix = blockIdx.x * kLabThreads + tid;
  const bool active = pix < plane;  // inactive lanes compute pixel 0 (they share the barriers), store nothing
  const int oy = active ? pix / a.ow : 0, ox = active ? pix % a.ow : 0;
  int ix[2] = {ox, ox}, iy[2] = {oy, oy};
  float wt[4] = {1.0f, 0.0f, 0.0f, 0.0f};
  if (NT == 4) {
    const double* ty = a.rec + a.axis_off + 3 * (int64_t)oy;
    const double* tx = a.rec + a.axis_off + 3 * (int64_t)(a.oh + ox);
    iy[0] = (int)ty[0];
    iy[1] = iy[0] + 1;
    ix[0] = (int)tx[0];
    ix[1] = ix[0] + 1;
    wt[0] = __double2float_rn(__dmul_rn(tx[1], ty[1]));
    wt[1] = __double2float_rn(__dmul_rn(tx[2], ty[1]));
    wt[2] = __double2float_rn(__dmul_rn(tx[1], ty[2]));
    wt[3] = __double2float_rn(__dmul_rn(tx[2], ty[2]));
  }
  const double gx[2] = {(double)ix[0], (double)ix[1]}, gy[2] = {(double)iy[0], (double)iy[1]};
  const int32_t* idx = a.idx + (int64_t)f * kLabGroups * 2;

  if (a.heat) {
    double all[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) all[t] = 0.0;
    for (int j = 0; j < OP_N_JOINTS; ++j) {
      const double* src = a.rec + idx[2 * j];
      const int cnt = idx[2 * j + 1];  // workgroup-uniform: so are the barriers below
      double m[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) m[t] = 0.0;
      for (int c0 = 0; c0 < cnt; c0 += kLabChunk) {
        const int nrec = min(kLabChunk, cnt - c0);
        __syncthreads();
        for (int i = tid; i < nrec * kJointRec; i += kLabThreads) srec[i] = src[(int64_t)c0 * kJointRec + i];
        __syncthreads();
        for (int r = 0; r < nrec; ++r) {
          const double x = srec[kJointRec * r], y = srec[kJointRec * r + 1];
          double dx2[2], dy2[2];
#pragma unroll
          for (int k = 0; k < (NT == 4 ? 2 : 1); ++k) {
            const double dx = __dsub_rn(gx[k], x), dy = __dsub_rn(gy[k], y);
            dx2[k] = __dmul_rn(dx, dx);
            dy2[k] = __dmul_rn(dy, dy);
          }
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const double d = __dadd_rn(dx2[t & 1], dy2[t >> 1]);
            const double e = exp(__ddiv_rn(__dmul_rn(-0.5, d), a.sigma2));
            m[t] = e > m[t] ? e : m[t];
          }
        }
      }
      float v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        all[t] = m[t] > all[t] ? m[t] : all[t];
        v[t] = __double2float_rn(m[t]);
      }
      if (active) a.heat[((int64_t)f * OP_N_HEAT + j) * plane + pix] = lab_combine<NT>(wt, v);
    }
    float v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = __double2float_rn(__dsub_rn(1.0, all[t]));  // background channel
    if (active) a.heat[((int64_t)f * OP_N_HEAT + OP_N_JOINTS) * plane + pix] = lab_combine<NT>(wt, v);
  }

  if (a.pafs) {
    for (int l = 0; l < OP_N_LIMBS; ++l) {
      const double* src = a.rec + idx[2 * (OP_N_JOINTS + l)];
      const int cnt = idx[2 * (OP_N_JOINTS + l) + 1];
      double sx[NT], sy[NT];
      int cn[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        sx[t] = 0.0;
        sy[t] = 0.0;
        cn[t] = 0;
      }
      for (int c0 = 0; c0 < cnt; c0 += kLabChunk) {
        const int nrec = min(kLabChunk, cnt - c0);
        __syncthreads();
        for (int i = tid; i < nrec * kLimbRec; i += kLabThreads) srec[i] = src[(int64_t)c0 * kLimbRec + i];
        __syncthreads();
        for (int r = 0; r < nrec; ++r) {
          const double* q = srec + kLimbRec * r;
          const double fx = q[0], fy = q[1], ux = q[2], uy = q[3], vx = q[4], vy = q[5], dist = q[6];
          double hx[2], hy[2], px[2], py[2];
#pragma unroll
          for (int k = 0; k < (NT == 4 ? 2 : 1); ++k) {
            const double ax = __dsub_rn(gx[k], fx), ay = __dsub_rn(gy[k], fy);
            hx[k] = __dmul_rn(ux, ax);
            hy[k] = __dmul_rn(uy, ay);
            px[k] = __dmul_rn(vx, ax);
            py[k] = __dmul_rn(vy, ay);
          }
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const double hip = __dadd_rn(hx[t & 1], hy[t >> 1]);
            const double vip = __dadd_rn(px[t & 1], py[t >> 1]);
            if (0.0 <= hip && hip <= dist && fabs(vip) <= a.paf_width) {  // people summed in person order
              sx[t] = __dadd_rn(sx[t], ux);
              sy[t] = __dadd_rn(sy[t], uy);
              ++cn[t];
            }
          }
        }
      }
      float vx4[NT], vy4[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        vx4[t] = __double2float_rn(cn[t] > 0 ? __ddiv_rn(sx[t], (double)cn[t]) : sx[t]);
        vy4[t] = __double2float_rn(cn[t] > 0 ? __ddiv_rn(sy[t], (double)cn[t]) : sy[t]);
      }
      if (active) {
        float* o = a.pafs + ((int64_t)f * OP_N_PAF + 2 * l) * plane + pix;
        o[0] = lab_combine<NT>(wt, vx4);
        o[plane] = lab_combine<NT>(wt, vy4);
      }
    }
  }

  if (a.ign && active) {
    // resize_images(mask.astype('f')) > 0: a tap counts when its f32 weight is non-zero
    bool v = false;
    if (a.mask) {
      const uint8_t* m = a.mask + (int64_t)f * a.h * a.w;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (wt[t] > 0.0f) v |= lab_dilated(m, a.h, a.w, iy[t >> 1], ix[t & 1]);
    }
    a.ign[(int64_t)f * plane + pix] = v ? 1 : 0;
  }
}

// linspace(0, L - 1, oL)[o] as NumPy forms it (oracle/postproc.c linspace_at), then the tap
void axis_tap_host(int o, int L, int oL, double* out) {
  const double stop = (double)(L - 1);
  double u;
  if (o == oL - 1) {
    u = stop;
  } else {
    const double step = stop / (double)(oL - 1);
    u = step == 0.0 ? ((double)o / (double)(oL - 1)) * stop : (double)o * step;
  }
  int i0 = (int)std::floor(u);
  i0 = i0 > L - 2 ? L - 2 : i0;
  i0 = i0 < 0 ? 0 : i0;
  out[0] = (double)i0;
  out[1] = (double)(i0 + 1) - u;
  out[2] = u - (double)i0;
}

}  // namespace

int labels_pack(const char* who, int32_t n, int32_t h, int32_t w, int32_t downscale, const double* poses,
                const int32_t* pose_offsets, double heatmap_sigma, double paf_width, LabelHost* out) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 16384 || w > 16384)
    return invalid(who, "bad shape (1 <= n <= 65535, 1 <= h, w <= 16384)");
  if (downscale < 1 || (downscale > 1 && (h % downscale || w % downscale || h / downscale < 2 || w / downscale < 2)))
    return invalid(who, "bad downscale (1, or a divisor of h and w with h/downscale, w/downscale >= 2)");
  if (!(heatmap_sigma > 0.0) || !std::isfinite(heatmap_sigma)) return invalid(who, "heatmap_sigma must be > 0");
  if (!(paf_width >= 0.0) || !std::isfinite(paf_width)) return invalid(who, "paf_width must be >= 0");
  if (!pose_offsets) return invalid(who, "null pose_offsets");
  if (pose_offsets[0] != 0) return invalid(who, "pose_offsets[0] must be 0");
  for (int f = 0; f < n; ++f)
    if (pose_offsets[f + 1] < pose_offsets[f]) return invalid(who, "pose_offsets must not decrease");
  const int64_t total = pose_offsets[n];
  if (total > (1 << 22)) return invalid(who, "too many people (the record offsets are 32-bit)");
  if (total > 0 && !poses) return invalid(who, "null poses with a non-zero person count");
  for (int64_t i = 0; i < total * OP_N_JOINTS * 3; ++i)
    if (!std::isfinite(poses[i])) return invalid(who, "non-finite pose value");

  op_params prm;
  op_default_params(&prm);  // limbs_point
  const double c = std::cos(M_PI / 2), s = std::sin(M_PI / 2);
  out->oh = h / downscale;
  out->ow = w / downscale;
  out->idx.assign((size_t)n * kLabGroups * 2, 0);
  out->rec.clear();
  for (int f = 0; f < n; ++f) {
    int32_t* idx = out->idx.data() + (size_t)f * kLabGroups * 2;
    const double* P = poses + (int64_t)pose_offsets[f] * OP_N_JOINTS * 3;
    const int np = pose_offsets[f + 1] - pose_offsets[f];
    for (int j = 0; j < OP_N_JOINTS; ++j) {
      idx[2 * j] = (int32_t)out->rec.size();
      for (int p = 0; p < np; ++p) {
        const double* q = P + ((int64_t)p * OP_N_JOINTS + j) * 3;
        if (q[2] > 0) {
          out->rec.push_back(q[0]);
          out->rec.push_back(q[1]);
          ++idx[2 * j + 1];
        }
      }
    }
    for (int l = 0; l < OP_N_LIMBS; ++l) {
      int32_t* e = idx + 2 * (OP_N_JOINTS + l);
      e[0] = (int32_t)out->rec.size();
      for (int p = 0; p < np; ++p) {
        const double* a = P + ((int64_t)p * OP_N_JOINTS + prm.limbs_point[l][0]) * 3;
        const double* b = P + ((int64_t)p * OP_N_JOINTS + prm.limbs_point[l][1]) * 3;
        if (!(a[2] > 0 && b[2] > 0) || (a[0] == b[0] && a[1] == b[1])) continue;
        const double dx = b[0] - a[0], dy = b[1] - a[1];
        const double dist = std::sqrt(dx * dx + dy * dy);
        const double ux = dx / dist, uy = dy / dist;
        const double rec[kLimbRec] = {a[0], a[1], ux, uy, c * ux + s * uy, -s * ux + c * uy, dist};
        out->rec.insert(out->rec.end(), rec, rec + kLimbRec);
        ++e[1];
      }
    }
  }
  out->axis_off = (int64_t)out->rec.size();
  if (downscale > 1) {
    double t[3];
    for (int o = 0; o < out->oh; ++o) {
      axis_tap_host(o, h, out->oh, t);
      out->rec.insert(out->rec.end(), t, t + 3);
    }
    for (int o = 0; o < out->ow; ++o) {
      axis_tap_host(o, w, out->ow, t);
      out->rec.insert(out->rec.end(), t, t + 3);
    }
  }
  if (out->rec.empty()) out->rec.push_back(0.0);  // never a zero-byte device buffer
  return OP_OK;
}

int launch_make_labels(const LabelHost& lh, const double* d_rec, const int32_t* d_idx, const uint8_t* d_mask,
                       int32_t n, int32_t h, int32_t w, int32_t downscale, double heatmap_sigma, double paf_width,
                       float* pafs, float* heat, uint8_t* ign, hipStream_t st) {
  LabelArgs a;
  a.rec = d_rec;
  a.idx = d_idx;
  a.mask = d_mask;
  a.h = h;
  a.w = w;
  a.oh = lh.oh;
  a.ow = lh.ow;
  a.axis_off = lh.axis_off;
  a.sigma2 = heatmap_sigma * heatmap_sigma;
  a.paf_width = paf_width;
  a.pafs = pafs;
  a.heat = heat;
  a.ign = ign;
  const dim3 grid((unsigned)((lh.oh * lh.ow + kLabThreads - 1) / kLabThreads), (unsigned)n);
  if (downscale == 1)
    hipLaunchKernelGGL(make_labels<1>, grid, dim3(kLabThreads), 0, st, a);
  else
    hipLaunchKernelGGL(make_labels<4>, grid, dim3(kLabThreads), 0, st, a);
  OP_AFTER_LAUNCH("make_labels", st);
  OP_HIP_CHECK(hipGetLastError());
  return OP_OK;
}

}  // namespace op

using namespace op;

extern "C" int op_make_labels(int32_t device, int32_t n, int32_t h, int32_t w, int32_t downscale, const double* poses,
                              const int32_t* pose_offsets, const uint8_t* mask, double heatmap_sigma,
                              double paf_width, float* pafs, float* heatmaps, uint8_t* ignore) {
  const char* who = "op_make_labels";
  LabelHost lh;
  int rc = labels_pack(who, n, h, w, downscale, poses, pose_offsets, heatmap_sigma, paf_width, &lh);
  if (rc) return rc;
  rc = use_device(who, device);
  if (rc) return rc;
  const size_t plane = (size_t)lh.oh * lh.ow;
  const size_t sizes[3] = {pafs ? n * OP_N_PAF * plane * sizeof(float) : 0,
                           heatmaps ? n * OP_N_HEAT * plane * sizeof(float) : 0, ignore ? n * plane : 0};
  void* host[3] = {pafs, heatmaps, ignore};
  Job job(who, nullptr);
  double* d_rec = (double*)job.alloc(lh.rec.size() * sizeof(double));
  int32_t* d_idx = (int32_t*)job.alloc(lh.idx.size() * sizeof(int32_t));
  uint8_t* d_mask = (uint8_t*)job.alloc(mask ? (size_t)n * h * w : 0);
  void* d_out[3];
  for (int i = 0; i < 3; ++i) d_out[i] = job.alloc(sizes[i]);
  job.upload(d_rec, lh.rec.data(), lh.rec.size() * sizeof(double), "records upload");
  job.upload(d_idx, lh.idx.data(), lh.idx.size() * sizeof(int32_t), "index upload");
  job.upload(d_mask, mask, mask ? (size_t)n * h * w : 0, "mask upload");
  if (job.ok()) {
    rc = launch_make_labels(lh, d_rec, d_idx, d_mask, n, h, w, downscale, heatmap_sigma, paf_width, (float*)d_out[0],
                            (float*)d_out[1], (uint8_t*)d_out[2], nullptr);
    if (rc) return rc;
  }
  job.finish("make_labels");
  for (int i = 0; i < 3; ++i) job.download(host[i], d_out[i], sizes[i]);
  return job.status();
}
