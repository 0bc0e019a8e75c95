// PAFs, heat maps and the ignore mask over a batch of frames (overlay.py: overlay_np is the statement,
// and the two agree bit for bit wherever the float64 atan2 lands in the same of its 256 hue levels).
//
// One kernel over the whole batch (overlay_tiles): one workgroup per 64 x 16 pixel tile of a frame, a
// thread owns four neighbouring pixels of a row, so it reads and writes 12 contiguous bytes (three
// dword accesses where the address is 4-byte aligned, bytes otherwise) and a wave four runs of 192.
// Per pixel, in the statement's order:
//   PAFs  every channel resampled to the frame (cv2.resize INTER_LINEAR on float32: the taps of
//         cvlinear.hpp's coordinate arithmetic, weights (1 - f, f), horizontal pass then vertical, one
//         rounded f32 operation each), the limbs summed in float64 in limb order onto +0.0, hue =
//         (atan2 / pi) / -2 + 0.5, saturation = value = min(sqrt(x x + y y), 1), * 255 truncated,
//         HSV2BGR as augment.hip's (OpenCV's f32 path), blended 0.6 / 0.4 in float64, rint to even;
//   heat  the f32 maximum over the resampled channels, * 255 clamped to 0 .. 255 and truncated, the
//         colour table's entry, blended alike;
//   mask  cv2.resize(mask * 255) > 0 in OpenCV's u8 fixed point (cvlinear.hpp): the pixel becomes 0.
// Maps are read through (channel, row, pixel) strides: planar (C, mh, mw) uploads and the precise
// path's sums, or the network's [row][col][channel] tensors in place.  Where a layer's maps are
// smaller than the frame in both directions, the window of source samples a tile's taps reach (about
// 10 x 4 for an 8x upsample) is staged once in LDS for all channels, if it fits beside the other
// layer's; otherwise (identity, downscaling, windows that do not fit) the taps are read from global
// memory.  Map sizes equal to the frame's are copied through, as the statement does.
// Every index is an integer formed from sizes alone or clamped by comparisons that are false for
// NaN: no map value can move a read outside the maps or the table.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "cvlinear.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kOvMaxSide = 16384;
constexpr int kOvThreads = 256;
constexpr int kOvTileW = 64, kOvTileH = 16, kOvPx = 4;  // kOvTileW / kOvPx threads per row, kOvTileH rows
constexpr int kOvLdsFloats = 3584;                      // 14 KiB of staged map windows per workgroup
constexpr int kOvHeatShown = 18;                        // op_overlay_staged: the joints, not the background

struct OvLayer {
  const float* p;              // sample (c, y, x) at p[c * cstr + y * rstr + x * pstr]
  int64_t cstr, rstr, pstr;
  int32_t c, mh, mw, pad;      // c = 0: no such layer
};
struct OvFrame {
  const uint8_t* src;
  uint8_t* dst;         // rows of 3 w bytes
  const uint8_t* mask;  // mkh x mkw bytes, nonzero = ignored; null: none
  int64_t src_stride;
  OvLayer paf, heat;
  int32_t h, w, mkh, mkw;
  int32_t tile0, tiles_x;  // the frame's first workgroup, tiles per row of tiles
};
struct OvArgs {
  const OvFrame* frames;
  const uint8_t* lut;  // 256 x 3 BGR; null when no frame has a heat layer
  int32_t n;
};

// cv2.resize INTER_LINEAR on float32: the taps of destination index d, clamped to the source
struct OvTap {
  int s0, s1;
  float w0, w1;
};

__device__ __forceinline__ OvTap ov_tap(int d, int dsize, int ssize) {
  const double inv = __ddiv_rn((double)dsize, (double)ssize);
  const double scale = __ddiv_rn(1.0, inv);
  float f = __double2float_rn(__dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5));
  int s = (int)floorf(f);
  f = __fsub_rn(f, (float)s);
  if (s < 0) {
    f = 0.0f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.0f;
    s = ssize - 1;
  }
  OvTap t;
  t.s0 = s;
  t.s1 = s + 1 < ssize ? s + 1 : ssize - 1;
  t.w0 = __fsub_rn(1.0f, f);
  t.w1 = f;
  return t;
}

// The source samples [x0, x0 + wx) x [y0, y0 + wy) of every channel, staged as [c][wy][wx].
struct OvWindow {
  int x0, y0, wx, wy;
  bool staged;
};

__device__ __forceinline__ OvWindow ov_window(const OvLayer& m, int h, int w, int tx0, int ty0, int tx1, int ty1,
                                              int room) {
  OvWindow v;
  v.x0 = v.y0 = v.wx = v.wy = 0;
  v.staged = false;
  if (m.c < 1 || m.mh >= h || m.mw >= w) return v;
  v.x0 = ov_tap(tx0, w, m.mw).s0;  // the taps never decrease along an axis
  v.y0 = ov_tap(ty0, h, m.mh).s0;
  v.wx = ov_tap(tx1, w, m.mw).s1 - v.x0 + 1;
  v.wy = ov_tap(ty1, h, m.mh).s1 - v.y0 + 1;
  v.staged = (int64_t)m.c * v.wx * v.wy <= (int64_t)room;
  return v;
}

__device__ __forceinline__ void ov_stage(const OvLayer& m, const OvWindow& v, float* s, int tid) {
  const int plane = v.wx * v.wy, total = m.c * plane;
  if (m.cstr == 1) {  // [row][col][channel] tensors: neighbouring lanes take neighbouring channels
    for (int i = tid; i < total; i += kOvThreads) {
      const int c = i % m.c, q = i / m.c, x = q % v.wx, y = q / v.wx;
      s[c * plane + y * v.wx + x] = m.p[(int64_t)c + (int64_t)(v.y0 + y) * m.rstr + (int64_t)(v.x0 + x) * m.pstr];
    }
  } else {
    for (int i = tid; i < total; i += kOvThreads) {
      const int x = i % v.wx, q = i / v.wx, y = q % v.wy, c = q / v.wy;
      s[i] = m.p[(int64_t)c * m.cstr + (int64_t)(v.y0 + y) * m.rstr + (int64_t)(v.x0 + x) * m.pstr];
    }
  }
}

struct OvLdsSrc {
  const float* s;
  int x0, y0, wx, plane;
  __device__ __forceinline__ float at(int c, int y, int x) const { return s[c * plane + (y - y0) * wx + (x - x0)]; }
};
struct OvGlobalSrc {
  const float* p;
  int64_t cstr, rstr, pstr;
  __device__ __forceinline__ float at(int c, int y, int x) const {
    return p[(int64_t)c * cstr + (int64_t)y * rstr + (int64_t)x * pstr];
  }
};

template <class Src>
__device__ __forceinline__ float ov_sample(const Src& src, int c, const OvTap& tx, const OvTap& ty, bool ident) {
  if (ident) return src.at(c, ty.s0, tx.s0);
  const float h0 = __fadd_rn(__fmul_rn(src.at(c, ty.s0, tx.s0), tx.w0), __fmul_rn(src.at(c, ty.s0, tx.s1), tx.w1));
  const float h1 = __fadd_rn(__fmul_rn(src.at(c, ty.s1, tx.s0), tx.w0), __fmul_rn(src.at(c, ty.s1, tx.s1), tx.w1));
  return __fadd_rn(__fmul_rn(h0, ty.w0), __fmul_rn(h1, ty.w1));
}

// overlay_pafs: the float64 sum of the limbs, in limb order, onto +0.0
template <class Src>
__device__ __forceinline__ void ov_mix(const Src& src, int limbs, bool ident, const OvTap* tx, const OvTap& ty,
                                       double* m0, double* m1) {
  for (int l = 0; l < limbs; ++l) {
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) {
      m0[p] = __dadd_rn(m0[p], (double)ov_sample(src, 2 * l, tx[p], ty, ident));
      m1[p] = __dadd_rn(m1[p], (double)ov_sample(src, 2 * l + 1, tx[p], ty, ident));
    }
  }
}

template <class Src>
__device__ __forceinline__ void ov_max(const Src& src, int channels, bool ident, const OvTap* tx, const OvTap& ty,
                                       float* mx) {
#pragma unroll
  for (int p = 0; p < kOvPx; ++p) mx[p] = ov_sample(src, 0, tx[p], ty, ident);
  for (int c = 1; c < channels; ++c) {
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) {
      const float v = ov_sample(src, c, tx[p], ty, ident);
      mx[p] = v > mx[p] ? v : mx[p];
    }
  }
}

// (v * 255).astype(uint8) of a value in [0, 1], clamped; false comparisons send NaN to 0
__device__ __forceinline__ int ov_level(double v) { return v >= 255.0 ? 255 : (v > 0.0 ? (int)v : 0); }

__device__ __forceinline__ int ov_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// overlay_paf's colour of the summed field (m0, m1): b | g << 8 | r << 16
__device__ __forceinline__ uint32_t ov_paf_colour(double m0, double m1) {
  const double hue = __dadd_rn(__ddiv_rn(__ddiv_rn(atan2(m1, m0), 3.141592653589793), -2.0), 0.5);
  double sat = __dsqrt_rn(__dadd_rn(__dmul_rn(m0, m0), __dmul_rn(m1, m1)));
  sat = sat > 1.0 ? 1.0 : sat;
  const int h = ov_level(__dmul_rn(hue, 255.0)), s = ov_level(__dmul_rn(sat, 255.0));
  // cv2.cvtColor HSV2BGR on u8 (H in 0..180; larger hues wrap), OpenCV's f32 path: augment.hsv2bgr_np
  float fh = __fmul_rn((float)h, __fdiv_rn(6.0f, 180.0f));
  const float fs = __fmul_rn((float)s, __fdiv_rn(1.0f, 255.0f));
  const float fv = fs;
  float o[3];
  if (s == 0) {
    o[0] = o[1] = o[2] = fv;
  } else {
    while (fh >= 6.0f) fh = __fsub_rn(fh, 6.0f);
    const int sector = ov_clampi((int)floorf(fh), 0, 5);
    fh = __fsub_rn(fh, (float)sector);
    float tab[4];
    tab[0] = fv;
    tab[1] = __fmul_rn(fv, __fsub_rn(1.0f, fs));
    tab[2] = __fmul_rn(fv, __fsub_rn(1.0f, __fmul_rn(fs, fh)));
    tab[3] = __fmul_rn(fv, __fsub_rn(1.0f, __fmul_rn(fs, __fsub_rn(1.0f, fh))));
    // sector_data {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}: two bits per entry, b | g << 2 | r << 4
    const unsigned codes = sector == 0   ? (1u | 3u << 2 | 0u << 4)
                           : sector == 1 ? (1u | 0u << 2 | 2u << 4)
                           : sector == 2 ? (3u | 0u << 2 | 1u << 4)
                           : sector == 3 ? (0u | 2u << 2 | 1u << 4)
                           : sector == 4 ? (0u | 1u << 2 | 3u << 4)
                                         : (2u | 1u << 2 | 0u << 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned k = (codes >> (2 * c)) & 3u;
      o[c] = k == 0 ? tab[0] : (k == 1 ? tab[1] : (k == 2 ? tab[2] : tab[3]));
    }
  }
  uint32_t out = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) out |= (uint32_t)ov_clampi(__float2int_rn(__fmul_rn(o[c], 255.0f)), 0, 255) << (8 * c);
  return out;
}

// demo.add_weighted(a, 0.6, b, 0.4, 0) on one channel
__device__ __forceinline__ uint32_t ov_blend_ch(uint32_t a, uint32_t b) {
  const double v = __dadd_rn(__dadd_rn(__dmul_rn((double)a, 0.6), __dmul_rn((double)b, 0.4)), 0.0);
  const double q = rint(v);  // half to even
  return q >= 255.0 ? 255u : (q > 0.0 ? (uint32_t)q : 0u);
}

__device__ __forceinline__ uint32_t ov_blend(uint32_t cur, uint32_t col) {
  return ov_blend_ch(cur & 255u, col & 255u) | (ov_blend_ch((cur >> 8) & 255u, (col >> 8) & 255u) << 8) |
         (ov_blend_ch((cur >> 16) & 255u, (col >> 16) & 255u) << 16);
}

__global__ __launch_bounds__(kOvThreads) void overlay_tiles(OvArgs a) {
  __shared__ float s_maps[kOvLdsFloats];
  __shared__ uint8_t s_lut[768];
  const int tid = threadIdx.x;
  int lo = 0, hi = a.n;  // the frame with tile0 <= blockIdx.x (no frame is without tiles)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.frames[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const OvFrame fr = a.frames[lo];
  const int tile = (int)blockIdx.x - fr.tile0;
  const int tx0 = (tile % fr.tiles_x) * kOvTileW, ty0 = (tile / fr.tiles_x) * kOvTileH;
  const int tx1 = min(tx0 + kOvTileW, fr.w) - 1, ty1 = min(ty0 + kOvTileH, fr.h) - 1;  // inclusive
  const OvWindow wp = ov_window(fr.paf, fr.h, fr.w, tx0, ty0, tx1, ty1, kOvLdsFloats);
  const int used = wp.staged ? fr.paf.c * wp.wx * wp.wy : 0;
  const OvWindow wh = ov_window(fr.heat, fr.h, fr.w, tx0, ty0, tx1, ty1, kOvLdsFloats - used);
  if (wp.staged) ov_stage(fr.paf, wp, s_maps, tid);
  if (wh.staged) ov_stage(fr.heat, wh, s_maps + used, tid);
  if (fr.heat.c > 0)
    for (int i = tid; i < 768; i += kOvThreads) s_lut[i] = a.lut[i];
  __syncthreads();
  const int x = tx0 + (tid % (kOvTileW / kOvPx)) * kOvPx, y = ty0 + tid / (kOvTileW / kOvPx);
  if (x > tx1 || y > ty1) return;  // (no barrier below)
  const int npx = min(kOvPx, tx1 - x + 1);
  uint32_t cur[kOvPx] = {0u, 0u, 0u, 0u};
  const uint8_t* sp = fr.src + (int64_t)y * fr.src_stride + (int64_t)x * 3;
  if (npx == kOvPx && ((uintptr_t)sp & 3u) == 0) {
    const uint32_t* sq = (const uint32_t*)sp;
    const uint32_t q0 = sq[0], q1 = sq[1], q2 = sq[2];
    cur[0] = q0 & 0xffffffu;
    cur[1] = (q0 >> 24) | ((q1 & 0xffffu) << 8);
    cur[2] = (q1 >> 16) | ((q2 & 0xffu) << 16);
    cur[3] = q2 >> 8;
  } else {
    for (int p = 0; p < npx; ++p)
      cur[p] = (uint32_t)sp[3 * p] | ((uint32_t)sp[3 * p + 1] << 8) | ((uint32_t)sp[3 * p + 2] << 16);
  }
  int xs[kOvPx];  // a thread past the frame's edge computes its last pixel again and stores none of it
#pragma unroll
  for (int p = 0; p < kOvPx; ++p) xs[p] = min(x + p, tx1);
  if (fr.paf.c > 0) {
    const OvLayer& m = fr.paf;
    const bool ident = m.mh == fr.h && m.mw == fr.w;
    OvTap tx[kOvPx];
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) tx[p] = ov_tap(xs[p], fr.w, m.mw);
    const OvTap ty = ov_tap(y, fr.h, m.mh);
    double m0[kOvPx] = {0.0, 0.0, 0.0, 0.0}, m1[kOvPx] = {0.0, 0.0, 0.0, 0.0};
    if (wp.staged)
      ov_mix(OvLdsSrc{s_maps, wp.x0, wp.y0, wp.wx, wp.wx * wp.wy}, m.c / 2, ident, tx, ty, m0, m1);
    else
      ov_mix(OvGlobalSrc{m.p, m.cstr, m.rstr, m.pstr}, m.c / 2, ident, tx, ty, m0, m1);
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) cur[p] = ov_blend(cur[p], ov_paf_colour(m0[p], m1[p]));
  }
  if (fr.heat.c > 0) {
    const OvLayer& m = fr.heat;
    const bool ident = m.mh == fr.h && m.mw == fr.w;
    OvTap tx[kOvPx];
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) tx[p] = ov_tap(xs[p], fr.w, m.mw);
    const OvTap ty = ov_tap(y, fr.h, m.mh);
    float mx[kOvPx];
    if (wh.staged)
      ov_max(OvLdsSrc{s_maps + used, wh.x0, wh.y0, wh.wx, wh.wx * wh.wy}, m.c, ident, tx, ty, mx);
    else
      ov_max(OvGlobalSrc{m.p, m.cstr, m.rstr, m.pstr}, m.c, ident, tx, ty, mx);
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) {
      const float v = __fmul_rn(mx[p], 255.0f);
      const int idx = v >= 255.0f ? 255 : (v > 0.0f ? (int)v : 0);
      const uint8_t* e = s_lut + idx * 3;
      cur[p] = ov_blend(cur[p], (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16));
    }
  }
  if (fr.mask) {  // cv2.resize(mask * 255, (w, h)) > 0: cvlinear.hpp's fixed point, columns clamped, rows not
    const LinTap ty = cv_linear_tap(y, fr.h, fr.mkh, false);
    const uint8_t* r0 = fr.mask + (int64_t)clampi(ty.s0, 0, fr.mkh - 1) * fr.mkw;
    const uint8_t* r1 = fr.mask + (int64_t)clampi(ty.s1, 0, fr.mkh - 1) * fr.mkw;
#pragma unroll
    for (int p = 0; p < kOvPx; ++p) {
      const LinTap tx = cv_linear_tap(xs[p], fr.w, fr.mkw, true);
      const int x0 = tx.s0, x1 = tx.s1 < fr.mkw ? tx.s1 : fr.mkw - 1;
      const int h0 = (r0[x0] ? 255 : 0) * tx.c0 + (r0[x1] ? 255 : 0) * tx.c1;
      const int h1 = (r1[x0] ? 255 : 0) * tx.c0 + (r1[x1] ? 255 : 0) * tx.c1;
      const int v = ((((h0 >> 4) * ty.c0) >> 16) + (((h1 >> 4) * ty.c1) >> 16) + 2) >> 2;
      if (clampi(v, 0, 255) > 0) cur[p] = 0u;
    }
  }
  uint8_t* dp = fr.dst + ((int64_t)y * fr.w + x) * 3;
  if (npx == kOvPx && ((uintptr_t)dp & 3u) == 0) {
    uint32_t* dq = (uint32_t*)dp;
    dq[0] = cur[0] | (cur[1] << 24);
    dq[1] = (cur[1] >> 8) | (cur[2] << 16);
    dq[2] = (cur[2] >> 16) | (cur[3] << 8);
  } else {
    for (int p = 0; p < npx; ++p) {
      dp[3 * p] = (uint8_t)(cur[p] & 255u);
      dp[3 * p + 1] = (uint8_t)((cur[p] >> 8) & 255u);
      dp[3 * p + 2] = (uint8_t)((cur[p] >> 16) & 255u);
    }
  }
}

// ---- host ----
// Lays the tiles of n frames (sizes set) out over the grid; makes no HIP call.
int ov_tiles(const char* who, std::vector<OvFrame>& frames, int64_t* tiles) {
  *tiles = 0;
  for (OvFrame& fr : frames) {
    fr.tiles_x = (fr.w + kOvTileW - 1) / kOvTileW;
    if (*tiles > INT32_MAX) break;
    fr.tile0 = (int32_t)*tiles;
    *tiles += (int64_t)fr.tiles_x * ((fr.h + kOvTileH - 1) / kOvTileH);
  }
  if (*tiles > INT32_MAX) return invalid(who, "hw: more than 2^31 - 1 pixel tiles in the batch");
  return OP_OK;
}

LastMs g_ov_last;

// The frame table and (with a heat layer) the colour table in the job's buffers
OvArgs ov_alloc(Job& job, int32_t n, bool any_heat) {
  OvArgs a;
  a.frames = (const OvFrame*)job.alloc((size_t)n * sizeof(OvFrame));
  a.lut = (const uint8_t*)job.alloc(any_heat ? 768 : 0);
  a.n = n;
  return a;
}

// Uploads the frames (src, dst and the layers set) and the colour table, queues overlay_tiles; ends
// the job's timing
void ov_run(Job& job, const std::vector<OvFrame>& frames, const uint8_t* lut, int64_t tiles, const OvArgs& a) {
  job.upload((void*)a.frames, frames.data(), frames.size() * sizeof(OvFrame));
  if (a.lut) job.upload((void*)a.lut, lut, 768);
  if (job.ok()) {
    hipLaunchKernelGGL(overlay_tiles, dim3((unsigned)tiles), dim3(kOvThreads), 0, job.stream(), a);
    job.check(hipGetLastError(), "overlay_tiles");
  }
  job.end();
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_overlay(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
                          const int32_t* hw, const float* const* pafs, const int32_t* paf_chw,
                          const float* const* heat, const int32_t* heat_chw, const uint8_t* const* mask,
                          const int32_t* mask_hw, const uint8_t* lut, uint8_t* const* out) {
  const char* who = "op_overlay";
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  RC(check_frames(who, n, bgr, row_stride, hw, out));
  if (pafs && !paf_chw) return invalid(who, "null paf_chw");
  if (heat && !heat_chw) return invalid(who, "null heat_chw");
  if (mask && !mask_hw) return invalid(who, "null mask_hw");
  auto side = [](int v) { return v >= 1 && v <= kOvMaxSide; };
  std::vector<OvFrame> frames((size_t)n);
  bool any_heat = false;
  for (int f = 0; f < n; ++f) {
    const std::string at = "frame " + std::to_string(f);
    OvFrame& fr = frames[f];
    memset(&fr, 0, sizeof(fr));
    fr.h = hw[2 * f];
    fr.w = hw[2 * f + 1];
    if (pafs && pafs[f]) {
      const int32_t* d = paf_chw + 3 * f;
      if (d[0] < 2 || d[0] % 2) return invalid(who, "paf_chw: " + at + ": a positive, even channel count expected");
      if (!side(d[1]) || !side(d[2])) return invalid(who, "paf_chw: " + at + ": mh, mw must be in 1 .. 16384");
      fr.paf.c = d[0];
      fr.paf.mh = d[1];
      fr.paf.mw = d[2];
    }
    if (heat && heat[f]) {
      const int32_t* d = heat_chw + 3 * f;
      if (d[0] < 1) return invalid(who, "heat_chw: " + at + ": a channel count of at least 1 expected");
      if (!side(d[1]) || !side(d[2])) return invalid(who, "heat_chw: " + at + ": mh, mw must be in 1 .. 16384");
      fr.heat.c = d[0];
      fr.heat.mh = d[1];
      fr.heat.mw = d[2];
      any_heat = true;
    }
    if (mask && mask[f]) {
      if (!side(mask_hw[2 * f]) || !side(mask_hw[2 * f + 1]))
        return invalid(who, "mask_hw: " + at + ": h, w must be in 1 .. 16384");
      fr.mkh = mask_hw[2 * f];
      fr.mkw = mask_hw[2 * f + 1];
    }
  }
  if (any_heat && !lut) return invalid(who, "null lut (a heat layer needs the 256 x 3 colour table)");
  int64_t tiles = 0;
  RC(ov_tiles(who, frames, &tiles));
  RC(use_device(who, device));
  // one buffer each for the frames in, the frames out (one layout: rows of 3 w bytes), the maps and the masks
  std::vector<int64_t> off(n + 1, 0), moff(2 * (size_t)n + 1, 0), koff(n + 1, 0);
  for (int f = 0; f < n; ++f) {
    const OvFrame& fr = frames[f];
    off[f + 1] = off[f] + pad16((int64_t)fr.h * fr.w * 3);
    moff[2 * f + 1] = moff[2 * f] + pad16((int64_t)fr.paf.c * fr.paf.mh * fr.paf.mw * 4);
    moff[2 * f + 2] = moff[2 * f + 1] + pad16((int64_t)fr.heat.c * fr.heat.mh * fr.heat.mw * 4);
    koff[f + 1] = koff[f] + pad16((int64_t)fr.mkh * fr.mkw);
  }
  Job job(who, nullptr);
  const OvArgs a = ov_alloc(job, n, any_heat);
  uint8_t* src = (uint8_t*)job.alloc((size_t)off[n]);
  uint8_t* dst = (uint8_t*)job.alloc((size_t)off[n]);
  const char* maps = (const char*)job.alloc((size_t)moff[2 * (size_t)n]);
  const uint8_t* masks = (const uint8_t*)job.alloc((size_t)koff[n]);
  job.begin();
  for (int f = 0; f < n && job.ok(); ++f) {
    OvFrame& fr = frames[f];
    fr.src = src + off[f];
    fr.dst = dst + off[f];
    fr.src_stride = (int64_t)fr.w * 3;
    job.upload2d((void*)fr.src, (size_t)fr.w * 3, bgr[f], (size_t)row_stride[f], (size_t)fr.w * 3, (size_t)fr.h,
                 "frame upload");
    OvLayer* layers[2] = {&fr.paf, &fr.heat};
    const float* host[2] = {fr.paf.c ? pafs[f] : nullptr, fr.heat.c ? heat[f] : nullptr};
    for (int k = 0; k < 2; ++k) {
      OvLayer& m = *layers[k];
      if (!m.c) continue;
      m.p = (const float*)(maps + moff[2 * f + k]);
      m.cstr = (int64_t)m.mh * m.mw;
      m.rstr = m.mw;
      m.pstr = 1;
      job.upload((void*)m.p, host[k], (size_t)m.c * m.mh * m.mw * 4, "map upload");
    }
    if (fr.mkh) {
      fr.mask = masks + koff[f];
      job.upload((void*)fr.mask, mask[f], (size_t)fr.mkh * fr.mkw, "mask upload");
    }
  }
  ov_run(job, frames, lut, tiles, a);
  job.finish("kernel");
  for (int f = 0; f < n; ++f) job.download(out[f], frames[f].dst, (size_t)frames[f].h * frames[f].w * 3);
  if (job.ok()) g_ov_last.done(device, job.ms());
  return job.status();
}

extern "C" int op_overlay_staged(op_ctx* c, int32_t first, int32_t n, int32_t layers, const uint8_t* lut,
                                 uint8_t* out) {
  const char* who = "op_overlay_staged";
  if (!c) return invalid(who, "null context");
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  if (!out) return invalid(who, "null out");
  if (layers & ~(OP_OVERLAY_PAFS | OP_OVERLAY_HEAT)) return invalid(who, "layers: unknown bits");
  if ((layers & OP_OVERLAY_HEAT) && !lut) return invalid(who, "null lut (the heat layer needs the 256 x 3 colour table)");
  RC(staged_range(c, who, first, n));
  if (c->st_h > kOvMaxSide || c->st_w > kOvMaxSide) return invalid(who, "staged frames above 16384 in h or w");
  RC(check_ctx(c, false));
  // the maps op_fetch_maps returns for these frames, where they lie
  int in_w, in_h, map_w, map_h;
  staged_sizes(c, &in_w, &in_h, &map_w, &map_h);
  const int mh = c->st_precise ? c->st_h : in_h / 8, mw = c->st_precise ? c->st_w : in_w / 8;
  const size_t mhw = (size_t)mh * mw, fbytes = (size_t)c->st_h * c->st_w * 3;
  const Act& m = c->split ? c->buf[B_MAP32] : c->buf[B_CAT];
  const bool have = c->st_precise ? (c->d_psum && c->psum_bytes >= (size_t)c->st_n * (OP_N_PAF + OP_N_HEAT) * mhw * 4)
                                  : (m.p && c->gn >= first + n && m.h == mh && m.w == mw);
  if (!have || mh < 1 || mw < 1 || mh > kOvMaxSide || mw > kOvMaxSide) {
    set_error("op_overlay_staged: no network maps of the staged frames (run op_run_staged first)");
    return OP_ERR_STATE;
  }
  std::vector<OvFrame> frames((size_t)n);
  for (int f = 0; f < n; ++f) {
    OvFrame& fr = frames[f];
    memset(&fr, 0, sizeof(fr));
    fr.h = c->st_h;
    fr.w = c->st_w;
    fr.src = c->d_frames + (size_t)(first + f) * fbytes;  // read in place
    fr.src_stride = (int64_t)c->st_w * 3;
    OvLayer paf, heat;
    memset(&paf, 0, sizeof(paf));
    paf.mh = mh;
    paf.mw = mw;
    heat = paf;
    if (c->st_precise) {  // the averaged maps: planar (57, h, w) per frame
      paf.p = c->d_psum + (size_t)(first + f) * (OP_N_PAF + OP_N_HEAT) * mhw;
      heat.p = paf.p + (size_t)OP_N_PAF * mhw;
      paf.cstr = heat.cstr = (int64_t)mhw;
      paf.rstr = heat.rstr = mw;
      paf.pstr = heat.pstr = 1;
    } else {  // the last-stage maps as the network wrote them: padded [row][col][channel]
      const int pw = mw + 2 * m.pad;
      const float* px = m.p + (size_t)(first + f) * m.frame_floats() + ((size_t)m.pad * pw + m.pad) * m.cs;
      paf.p = px + (c->split ? 0 : kCatPaf);
      heat.p = px + (c->split ? 40 : kCatHeat);
      paf.cstr = heat.cstr = 1;
      paf.rstr = heat.rstr = (int64_t)pw * m.cs;
      paf.pstr = heat.pstr = m.cs;
    }
    paf.c = OP_N_PAF;
    heat.c = kOvHeatShown;
    if (layers & OP_OVERLAY_PAFS) fr.paf = paf;
    if (layers & OP_OVERLAY_HEAT) fr.heat = heat;
  }
  int64_t tiles = 0;
  RC(ov_tiles(who, frames, &tiles));
  Job job(who, c->stream);  // everything is ordered on the context stream, behind a queued run
  const OvArgs a = ov_alloc(job, n, (layers & OP_OVERLAY_HEAT) != 0);
  uint8_t* dst = (uint8_t*)job.alloc(fbytes * n);
  for (int f = 0; f < n && job.ok(); ++f) frames[f].dst = dst + (size_t)f * fbytes;
  job.begin();
  ov_run(job, frames, lut, tiles, a);
  job.download(out, dst, fbytes * n);
  if (job.finish("kernel") == OP_OK) g_ov_last.done(c->device, job.ms());
  return job.status();
}

extern "C" int op_overlay_last_ms(int32_t device, double* ms) {
  return g_ov_last.get("op_overlay_last_ms", "op_overlay or op_overlay_staged", device, ms);
}
