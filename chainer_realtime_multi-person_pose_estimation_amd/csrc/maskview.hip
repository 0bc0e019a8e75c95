// The --vis viewer of gen_ignore_mask.py on the device: per frame the annotation view
// (draw_masks_and_keypoints, :48-71) and the mask_miss view (dwaw_gen_masks, :39-46).  maskview.py's
// view_np is the statement, and the two agree byte for byte.
//
// Host (op_annotation_views): every argument is validated before the first HIP call; the
// segmentation arguments go through masks.hip's mask_pack, the keypoints with v = 1 or 2 become
// discs (centre, colour) in order, the others leave the list.  masks.hip's three kernels then leave
// every annotation's mask and every frame's mask_miss in HBM as row-major u8; no mask visits the host.
// Device, one kernel over the whole batch (view_tiles): one workgroup per 64 x 16 pixel tile of a
// frame, a thread owns four neighbouring pixels of a row (12 contiguous bytes: three dword accesses
// where the address is 4-byte aligned, bytes otherwise) and keeps their three channels as float64 in
// registers, the reference's carried float image.  It walks the frame's annotations in order:
//   the tint   where the annotation's mask covers the pixel, per channel
//              v = (v + 0.7 * c * 255) - 0.7 * v, c = 1 on the channel the tint code names and 0 on
//              the others: __dmul_rn / __dadd_rn / __dsub_rn, one rounding each, in that order;
//   the discs  in chunks of 256: a lane tests one disc's box against the tile, the survivors are
//              compacted in order into LDS (wave ballot, prefix by popcount, wave totals through LDS),
//              and every pixel walks them from the back and stops at its first hit (draw.hip's integer
//              test, radius 3): the last disc that hits wins, and a later chunk overwrites an earlier
//              one.  A hit sets the three channels to the disc's colour (255.0 / 0.0).
// The cast at the end is truncation, as astype(uint8) is for values in [0, 256).
//
// Skipping the tint where the mask is clear is exact.  The statement computes there, per channel,
// (v + 0.7 * 0.0) - 0.7 * (v * 0) = (v + 0.0) - 0.0, and v + 0.0 == v and v - 0.0 == v bit for bit
// for every v that is not -0.0.  No v is: a frame byte is >= +0, a disc writes 255.0 or +0.0, and a
// tint maps v >= +0 to fl(fl(v + t) - fl(0.7 v)) with t >= 0, where fl(0.7 v) <= v <= fl(v + t) by the
// monotonicity of rounding, so the difference is >= 0 and, when zero, +0.0 under round-to-nearest.
// The same bounds keep v below 255.5 (tests/test_maskview_host.py iterates them), so the truncating
// cast never wraps.  mask_miss's view is the same step once, on the frame's bytes.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "masks.hpp"

namespace op {
namespace {

constexpr int kViewMaxCoord = 32768;
constexpr int kViewThreads = 256;
constexpr int kViewChunk = kViewThreads;  // discs per pass: one per lane
constexpr int kViewTileW = 64, kViewTileH = 16, kViewPx = 4;  // 16 threads x 4 pixels per row, 16 rows
constexpr int kViewRadius = 3;
constexpr double kViewAlpha = 0.7;

struct ViewFrame {
  const uint8_t* src;
  uint8_t* dst_ann;     // rows of 3 w bytes; null: not wanted
  uint8_t* dst_miss;    // alike
  const uint8_t* miss;  // the frame's mask_miss, rows of w bytes
  int64_t src_stride;
  int32_t h, w;
  int32_t ann0, ann1;
  int32_t tile0, tiles_x;  // the frame's first workgroup, tiles per row of tiles
};
struct ViewAnn {
  const uint8_t* mask;  // rows of w bytes
  int32_t tint;         // the channel the tint raises
  int32_t kp0, kp1;     // its discs
  int32_t pad;
};
struct ViewDisc {
  int32_t x, y;
  uint32_t col, pad;  // b | g << 8 | r << 16
};
struct ViewArgs {
  const ViewFrame* frames;
  const ViewAnn* anns;
  const ViewDisc* discs;
  int32_t n;
};

// four bytes from p (the first cnt of them are inside the row), one per byte of the result
__device__ __forceinline__ uint32_t view_load4(const uint8_t* p, int cnt) {
  if (cnt == 4 && ((uintptr_t)p & 3u) == 0) return *(const uint32_t*)p;
  uint32_t v = 0u;
  for (int q = 0; q < cnt; ++q) v |= (uint32_t)p[q] << (8 * q);
  return v;
}

// twelve bytes of a row, as three bytes per entry of px (the first npx entries are inside the row)
__device__ __forceinline__ void view_load12(const uint8_t* p, int npx, uint32_t* px) {
  if (npx == kViewPx && ((uintptr_t)p & 3u) == 0) {
    const uint32_t* q = (const uint32_t*)p;
    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
    px[0] = q0 & 0xffffffu;
    px[1] = (q0 >> 24) | ((q1 & 0xffffu) << 8);
    px[2] = (q1 >> 16) | ((q2 & 0xffu) << 16);
    px[3] = q2 >> 8;
  } else {
    for (int k = 0; k < kViewPx; ++k)
      px[k] = k < npx ? (uint32_t)p[3 * k] | ((uint32_t)p[3 * k + 1] << 8) | ((uint32_t)p[3 * k + 2] << 16) : 0u;
  }
}

__device__ __forceinline__ void view_store12(uint8_t* p, int npx, const uint32_t* px) {
  if (npx == kViewPx && ((uintptr_t)p & 3u) == 0) {
    uint32_t* q = (uint32_t*)p;
    q[0] = px[0] | (px[1] << 24);
    q[1] = (px[1] >> 8) | (px[2] << 16);
    q[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    for (int k = 0; k < npx; ++k) {
      p[3 * k] = (uint8_t)(px[k] & 255u);
      p[3 * k + 1] = (uint8_t)((px[k] >> 8) & 255u);
      p[3 * k + 2] = (uint8_t)((px[k] >> 16) & 255u);
    }
  }
}

// one step of the reference on a covered pixel's channel: (v + 0.7 * c * 255) - 0.7 * v
__device__ __forceinline__ double view_tint(double v, bool raised) {
  const double t = raised ? __dmul_rn(kViewAlpha, 255.0) : 0.0;
  return __dsub_rn(__dadd_rn(v, t), __dmul_rn(kViewAlpha, v));
}

__global__ __launch_bounds__(kViewThreads) void view_tiles(ViewArgs a) {
  __shared__ int32_t s_x[kViewChunk], s_y[kViewChunk];
  __shared__ uint32_t s_col[kViewChunk];
  __shared__ int32_t s_cnt[kViewThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int lo = 0, hi = a.n;  // the frame with tile0 <= blockIdx.x (no frame is without tiles)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.frames[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const ViewFrame fr = a.frames[lo];
  const int tile = (int)blockIdx.x - fr.tile0;
  const int tx0 = (tile % fr.tiles_x) * kViewTileW, ty0 = (tile / fr.tiles_x) * kViewTileH;
  const int tx1 = min(tx0 + kViewTileW, fr.w) - 1, ty1 = min(ty0 + kViewTileH, fr.h) - 1;  // inclusive
  const int x = tx0 + (tid % (kViewTileW / kViewPx)) * kViewPx, y = ty0 + tid / (kViewTileW / kViewPx);
  const bool in = x <= tx1 && y <= ty1;  // (the barriers below need every thread)
  const int npx = in ? min(kViewPx, tx1 - x + 1) : 0;
  uint32_t orig[kViewPx] = {0u, 0u, 0u, 0u};
  if (in) view_load12(fr.src + (int64_t)y * fr.src_stride + (int64_t)x * 3, npx, orig);
  if (fr.dst_ann) {
    double st[kViewPx][3];
#pragma unroll
    for (int k = 0; k < kViewPx; ++k) {
      st[k][0] = (double)(orig[k] & 255u);
      st[k][1] = (double)((orig[k] >> 8) & 255u);
      st[k][2] = (double)((orig[k] >> 16) & 255u);
    }
    for (int ai = fr.ann0; ai < fr.ann1; ++ai) {
      const ViewAnn an = a.anns[ai];
      if (in) {
        const uint32_t m = view_load4(an.mask + (int64_t)y * fr.w + x, npx);
#pragma unroll
        for (int k = 0; k < kViewPx; ++k)
          if ((m >> (8 * k)) & 255u) {
            st[k][0] = view_tint(st[k][0], an.tint == 0);
            st[k][1] = view_tint(st[k][1], an.tint == 1);
            st[k][2] = view_tint(st[k][2], an.tint == 2);
          }
      }
      for (int base = an.kp0; base < an.kp1; base += kViewChunk) {
        const int i = base + tid;
        ViewDisc dc;
        bool keep = false;
        if (i < an.kp1) {
          dc = a.discs[i];
          keep = dc.x - kViewRadius <= tx1 && dc.x + kViewRadius >= tx0 && dc.y - kViewRadius <= ty1 &&
                 dc.y + kViewRadius >= ty0;
        }
        const unsigned long long bal = __ballot((int)keep);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < kViewThreads / 64; ++v) {
          const int c = s_cnt[v];
          if (v < wave) pos += c;
          total += c;
        }
        if (keep) {  // pos < total <= kViewChunk
          s_x[pos] = dc.x;
          s_y[pos] = dc.y;
          s_col[pos] = dc.col;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kViewPx; ++k) {
          if (k >= npx) continue;
          for (int j = total - 1; j >= 0; --j) {  // |ddx|, |ddy| <= 32768 + 16384: the squares fit int32 once boxed
            const int ddx = x + k - s_x[j], ddy = y - s_y[j];
            if (ddx < -kViewRadius || ddx > kViewRadius || ddy < -kViewRadius || ddy > kViewRadius) continue;
            if (ddx * ddx + ddy * ddy <= kViewRadius * kViewRadius) {
              const uint32_t col = s_col[j];
              st[k][0] = (double)(col & 255u);
              st[k][1] = (double)((col >> 8) & 255u);
              st[k][2] = (double)((col >> 16) & 255u);
              break;
            }
          }
        }
        __syncthreads();  // the next chunk overwrites the list
      }
    }
    if (in) {
      uint32_t px[kViewPx];
#pragma unroll
      for (int k = 0; k < kViewPx; ++k)  // 0 <= st < 255.5: truncation, as astype(uint8)
        px[k] = (uint32_t)st[k][0] | ((uint32_t)st[k][1] << 8) | ((uint32_t)st[k][2] << 16);
      view_store12(fr.dst_ann + ((int64_t)y * fr.w + x) * 3, npx, px);
    }
  }
  if (fr.dst_miss && in) {
    const uint32_t m = view_load4(fr.miss + (int64_t)y * fr.w + x, npx);
    uint32_t px[kViewPx];
#pragma unroll
    for (int k = 0; k < kViewPx; ++k) {
      px[k] = orig[k];
      if ((m >> (8 * k)) & 255u)  // dwaw_gen_masks' colour (0, 0, 1): the tint raises channel 2
        px[k] = (uint32_t)view_tint((double)(orig[k] & 255u), false) |
                ((uint32_t)view_tint((double)((orig[k] >> 8) & 255u), false) << 8) |
                ((uint32_t)view_tint((double)((orig[k] >> 16) & 255u), true) << 16);
    }
    view_store12(fr.dst_miss + ((int64_t)y * fr.w + x) * 3, npx, px);
  }
}

// ---- host ----
LastMs g_view_last;

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_annotation_views(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
                                   const int32_t* hw, const int32_t* ann_offsets, const int32_t* ann_role,
                                   const int32_t* ann_tint, const int32_t* part_offsets, const int32_t* part_kind,
                                   const int64_t* data_offsets, const double* xy, const uint32_t* counts,
                                   const int32_t* kp_offsets, const int32_t* kp, uint8_t* const* out_ann,
                                   uint8_t* const* out_miss) {
  const char* who = "op_annotation_views";
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  if (!bgr) return invalid(who, "null bgr");
  if (!row_stride) return invalid(who, "null row_stride");
  MaskHost mh;
  int rc = mask_pack(who, n, hw, ann_offsets, ann_role, part_offsets, part_kind, data_offsets, xy, counts, nullptr,
                     out_ann, &mh);
  if (rc) return rc;
  std::vector<ViewFrame> frames(n);
  int64_t tiles = 0;
  for (int f = 0; f < n; ++f) {
    const std::string at = "frame " + std::to_string(f);
    ViewFrame& fr = frames[f];
    memset(&fr, 0, sizeof(fr));
    fr.h = hw[2 * f];
    fr.w = hw[2 * f + 1];
    if (!bgr[f]) return invalid(who, "bgr: " + at + ": null image");
    if (row_stride[f] < (int64_t)fr.w * 3) return invalid(who, "row_stride: " + at + ": fewer than 3 w bytes per row");
    fr.ann0 = ann_offsets[f];
    fr.ann1 = ann_offsets[f + 1];
    fr.tiles_x = (fr.w + kViewTileW - 1) / kViewTileW;
    fr.tile0 = (int32_t)tiles;
    tiles += (int64_t)fr.tiles_x * ((fr.h + kViewTileH - 1) / kViewTileH);
    if (tiles > INT32_MAX) return invalid(who, "more than 2^31 - 1 pixel tiles in the batch");
  }
  const int32_t A = ann_offsets[n];
  if (A > 0 && !ann_tint) return invalid(who, "null ann_tint");
  for (int a = 0; a < A; ++a)
    if (ann_tint[a] != OP_VIEW_PERSON && ann_tint[a] != OP_VIEW_NO_KEYPOINTS && ann_tint[a] != OP_VIEW_CROWD)
      return invalid(who, "ann_tint: annotation " + std::to_string(a) + ": unknown tint " + std::to_string(ann_tint[a]));
  rc = mask_offsets(who, "kp_offsets", nullptr, kp_offsets, A);
  if (rc) return rc;
  const int32_t K = kp_offsets[A];
  if (K > 0 && !kp) return invalid(who, "null kp");
  for (int i = 0; i < K; ++i)
    for (int c = 0; c < 2; ++c)
      if (kp[3 * i + c] < -kViewMaxCoord || kp[3 * i + c] > kViewMaxCoord)
        return invalid(who, "kp: keypoint " + std::to_string(i) + ": a coordinate above 32768 in magnitude");
  // everything is valid: the discs of the keypoints with v = 1 or 2, in order
  std::vector<ViewAnn> anns(A);
  std::vector<ViewDisc> discs;
  for (int a = 0; a < A; ++a) {
    ViewAnn& an = anns[a];
    memset(&an, 0, sizeof(an));
    an.tint = ann_tint[a];
    an.kp0 = (int32_t)discs.size();
    for (int i = kp_offsets[a]; i < kp_offsets[a + 1]; ++i) {
      const int32_t v = kp[3 * i + 2];
      if (v != 1 && v != 2) continue;
      discs.push_back(ViewDisc{kp[3 * i], kp[3 * i + 1], v == 1 ? 0x00ffffu : 0xff00ffu, 0u});  // (255, 255, 0) / (255, 0, 255)
    }
    an.kp1 = (int32_t)discs.size();
  }
  rc = use_device(who, device);
  if (rc) return rc;
  std::vector<int64_t> off(n + 1, 0);  // source and destination frames share one layout: rows of 3 w bytes
  bool want_ann = false, want_miss = false;
  for (int f = 0; f < n; ++f) {
    off[f + 1] = off[f] + pad16((int64_t)frames[f].h * frames[f].w * 3);
    want_ann = want_ann || (out_ann && out_ann[f]);
    want_miss = want_miss || (out_miss && out_miss[f]);
  }
  Job job(who, nullptr);
  ViewArgs a;
  a.frames = (const ViewFrame*)job.alloc(frames.size() * sizeof(ViewFrame));
  a.anns = (const ViewAnn*)job.alloc(anns.size() * sizeof(ViewAnn));
  a.discs = (const ViewDisc*)job.alloc(discs.size() * sizeof(ViewDisc));
  a.n = n;
  uint8_t* src = (uint8_t*)job.alloc((size_t)off[n]);
  uint8_t* dann = (uint8_t*)job.alloc(want_ann ? (size_t)off[n] : 0);
  uint8_t* dmiss = (uint8_t*)job.alloc(want_miss ? (size_t)off[n] : 0);
  MaskDevice md;
  mask_launch(job, mh, &md);  // the masks: masks.hip's kernels, queued on the null stream ahead of view_tiles
  for (int f = 0; f < n && job.ok(); ++f) {
    ViewFrame& fr = frames[f];
    fr.src = src + off[f];
    fr.src_stride = (int64_t)fr.w * 3;
    fr.dst_ann = out_ann && out_ann[f] ? dann + off[f] : nullptr;
    fr.dst_miss = out_miss && out_miss[f] ? dmiss + off[f] : nullptr;
    fr.miss = md.miss() + mh.images[f].out_off;
    for (int k = fr.ann0; k < fr.ann1; ++k)  // out_off >= 0 wherever dst_ann is set
      anns[k].mask = mh.anns[k].out_off >= 0 ? md.ann() + mh.anns[k].out_off : nullptr;
    job.upload2d((void*)fr.src, (size_t)fr.w * 3, bgr[f], (size_t)row_stride[f], (size_t)fr.w * 3, (size_t)fr.h,
                 "frame upload");
  }
  job.upload((void*)a.frames, frames.data(), frames.size() * sizeof(ViewFrame));
  job.upload((void*)a.anns, anns.data(), anns.size() * sizeof(ViewAnn));
  job.upload((void*)a.discs, discs.data(), discs.size() * sizeof(ViewDisc));
  if (job.ok()) {
    hipLaunchKernelGGL(view_tiles, dim3((unsigned)tiles), dim3(kViewThreads), 0, nullptr, a);
    job.check(hipGetLastError(), "view_tiles");
  }
  job.end();
  job.finish("kernels");
  for (int f = 0; f < n; ++f) {
    const size_t bytes = (size_t)frames[f].h * frames[f].w * 3;
    if (frames[f].dst_ann) job.download(out_ann[f], frames[f].dst_ann, bytes);
    if (frames[f].dst_miss) job.download(out_miss[f], frames[f].dst_miss, bytes);
  }
  if (job.ok()) g_view_last.done(device, job.ms());
  return job.status();
}

extern "C" int op_annotation_views_last_ms(int32_t device, double* ms) {
  return g_view_last.get("op_annotation_views_last_ms", "op_annotation_views", device, ms);
}
