// Skeleton overlays on the device: a batch of frames, each with a display list of lines, discs and
// at most one blend marker (render.py builds the lists; render_np is the statement, and the two
// agree bit for bit).
//
// Host (draw_pack, plain double operations, no contraction): every argument is validated; per line
// r = thickness / 2, the box floor(min - r) .. ceil(max + r), dx, dy, n2 = dx dx + dy dy and r r, as
// draw.draw_line computes them; per disc the box centre -+ radius.  The blend marker leaves the
// list: a frame keeps the index it stood at and its three weights.
// Device, one kernel over the whole batch (draw_tiles): one workgroup per 64 x 16 pixel tile of a
// frame, a thread owns the pixels (x, y), (x, y + 4), (x, y + 8), (x, y + 12), so a wave reads and
// writes 192 contiguous bytes of a row.  The list is walked in chunks of 256: a lane tests one
// primitive's box (16 bytes, an array of its own) against the tile, and a line's distance from the
// tile's centre (a conservative cull: kDrawReach); the survivors are compacted in order into LDS
// (wave ballot, prefix by popcount, wave totals through LDS), and every pixel walks the chunk's
// survivors from the back and stops at its first hit: the last writer wins, and a later chunk
// overwrites an earlier one.  The primitives before the blend marker are walked first, then the blend of the
// input pixel and the picture so far, then the primitives after it.
// The line test restates draw.draw_line one rounded float64 operation at a time (__dmul_rn,
// __dadd_rn, __ddiv_rn) in its order; the box is part of the test.  The disc test is integer.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kDrawMaxSide = 16384;
constexpr double kDrawMaxCoord = 32768.0;
constexpr int kDrawMaxRadius = 1024;
constexpr int kDrawThreads = 256;
constexpr int kDrawChunk = kDrawThreads;  // primitives per pass: one per lane
constexpr int kDrawTileW = 64, kDrawTileH = 16, kDrawRows = kDrawTileH / (kDrawThreads / kDrawTileW);
// A line paints a pixel of a tile only if the tile's centre lies within r + kDrawReach of the
// segment: half the tile's diagonal (31.5, 7.5: 32.4) and a pixel of slack for every rounding of
// the two distance computations (coordinates are at most 32768: their errors are below 1e-9).
constexpr double kDrawReach = 33.5;
constexpr uint32_t kDrawDiscBit = 1u << 24;  // in DrawRec::col above the three colour bytes

struct DrawBox {
  int32_t lx, hx, ly, hy;  // inclusive (a disc's: centre -+ radius)
};
struct DrawRec {
  double x0, y0, dx, dy, n2, r2;  // a line's; a disc reads none
  double cull2;                   // a line's: (r + kDrawReach)^2
  uint32_t col, pad;              // b | g << 8 | r << 16 | kDrawDiscBit
};
struct DrawFrame {
  const uint8_t* src;
  uint8_t* dst;  // rows of 3 w bytes
  int64_t src_stride;
  double wa, wb, gamma;
  int32_t h, w;
  int32_t p0, pb, p1;  // records [p0, pb) before the blend, [pb, p1) after it (no blend: pb = p1)
  int32_t blend;
  int32_t tile0, tiles_x;  // the frame's first workgroup, tiles per row of tiles
};
struct DrawArgs {
  const DrawFrame* frames;
  const DrawBox* boxes;  // by record: the cull reads these 16 bytes alone
  const DrawRec* recs;   // read by the survivors
  int32_t n;
};

__device__ __forceinline__ uint32_t draw_blend_ch(uint32_t a, uint32_t b, double wa, double wb, double gamma) {
  const double v = __dadd_rn(__dadd_rn(__dmul_rn((double)a, wa), __dmul_rn((double)b, wb)), gamma);
  const double q = rint(v);  // half to even
  return q >= 255.0 ? 255u : (q > 0.0 ? (uint32_t)q : 0u);
}

__global__ __launch_bounds__(kDrawThreads) void draw_tiles(DrawArgs a) {
  __shared__ double s_x0[kDrawChunk], s_y0[kDrawChunk], s_dx[kDrawChunk], s_dy[kDrawChunk], s_n2[kDrawChunk],
      s_r2[kDrawChunk];
  __shared__ int32_t s_lx[kDrawChunk], s_hx[kDrawChunk], s_ly[kDrawChunk], s_hy[kDrawChunk];
  __shared__ uint32_t s_col[kDrawChunk];
  __shared__ int32_t s_cnt[kDrawThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int lo = 0, hi = a.n;  // the frame with tile0 <= blockIdx.x (no frame is without tiles)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.frames[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const DrawFrame fr = a.frames[lo];
  const int tile = (int)blockIdx.x - fr.tile0;
  const int tx0 = (tile % fr.tiles_x) * kDrawTileW, ty0 = (tile / fr.tiles_x) * kDrawTileH;
  const int tx1 = min(tx0 + kDrawTileW, fr.w) - 1, ty1 = min(ty0 + kDrawTileH, fr.h) - 1;  // inclusive
  const int x = tx0 + lane;
  const double fx = (double)x;
  uint32_t orig[kDrawRows], cur[kDrawRows];
  bool in[kDrawRows];
#pragma unroll
  for (int k = 0; k < kDrawRows; ++k) {
    const int y = ty0 + wave + k * (kDrawThreads / kDrawTileW);
    in[k] = x <= tx1 && y <= ty1;
    orig[k] = 0u;
    if (in[k]) {
      const uint8_t* p = fr.src + (int64_t)y * fr.src_stride + (int64_t)x * 3;
      orig[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    cur[k] = orig[k];
  }
  for (int seg = 0; seg < 2; ++seg) {
    const int s0 = seg ? fr.pb : fr.p0, s1 = seg ? fr.p1 : fr.pb;
    for (int base = s0; base < s1; base += kDrawChunk) {
      const int i = base + tid;
      DrawBox box;
      DrawRec rec;
      bool keep = false;
      if (i < s1) {
        box = a.boxes[i];
        if (box.lx <= tx1 && box.hx >= tx0 && box.ly <= ty1 && box.hy >= ty0) {
          rec = a.recs[i];
          keep = true;
          if (!(rec.col & kDrawDiscBit)) {  // a long slanted line's box holds tiles far from the line
            const double cx = (double)tx0 + 0.5 * (kDrawTileW - 1), cy = (double)ty0 + 0.5 * (kDrawTileH - 1);
            double t = 0.0;
            if (rec.n2 > 0.0) {
              t = ((cx - rec.x0) * rec.dx + (cy - rec.y0) * rec.dy) / rec.n2;
              t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            }
            const double ex = cx - (rec.x0 + t * rec.dx), ey = cy - (rec.y0 + t * rec.dy);
            keep = ex * ex + ey * ey <= rec.cull2;
          }
        }
      }
      const unsigned long long bal = __ballot((int)keep);
      if (lane == 0) s_cnt[wave] = __popcll(bal);
      __syncthreads();
      int pos = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
      for (int v = 0; v < kDrawThreads / 64; ++v) {
        const int c = s_cnt[v];
        if (v < wave) pos += c;
        total += c;
      }
      if (keep) {  // pos < total <= kDrawChunk
        s_x0[pos] = rec.x0;
        s_y0[pos] = rec.y0;
        s_dx[pos] = rec.dx;
        s_dy[pos] = rec.dy;
        s_n2[pos] = rec.n2;
        s_r2[pos] = rec.r2;
        s_lx[pos] = box.lx;
        s_hx[pos] = box.hx;
        s_ly[pos] = box.ly;
        s_hy[pos] = box.hy;
        s_col[pos] = rec.col;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kDrawRows; ++k) {
        if (!in[k]) continue;
        const int y = ty0 + wave + k * (kDrawThreads / kDrawTileW);
        const double fy = (double)y;
        for (int j = total - 1; j >= 0; --j) {
          const int lx = s_lx[j], hx = s_hx[j], ly = s_ly[j], hy = s_hy[j];
          if (x < lx || x > hx || y < ly || y > hy) continue;
          const uint32_t col = s_col[j];
          bool hit;
          if (col & kDrawDiscBit) {  // lx + hx = 2 cx, hx - lx = 2 radius; |ddx|, |ddy| <= radius <= 1024
            const int ddx = x - (lx + hx) / 2, ddy = y - (ly + hy) / 2, rad = (hx - lx) / 2;
            hit = ddx * ddx + ddy * ddy <= rad * rad;
          } else {
            const double x0 = s_x0[j], y0 = s_y0[j], dx = s_dx[j], dy = s_dy[j], n2 = s_n2[j];
            double t = 0.0;
            if (n2 > 0.0) {
              t = __ddiv_rn(__dadd_rn(__dmul_rn(__dsub_rn(fx, x0), dx), __dmul_rn(__dsub_rn(fy, y0), dy)), n2);
              t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            }
            const double ex = __dsub_rn(fx, __dadd_rn(x0, __dmul_rn(t, dx)));
            const double ey = __dsub_rn(fy, __dadd_rn(y0, __dmul_rn(t, dy)));
            hit = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)) <= s_r2[j];
          }
          if (hit) {
            cur[k] = col & 0xffffffu;
            break;
          }
        }
      }
      __syncthreads();  // the next chunk overwrites the list
    }
    if (seg == 0 && fr.blend) {
#pragma unroll
      for (int k = 0; k < kDrawRows; ++k) {
        const uint32_t o = orig[k], c = cur[k];
        cur[k] = draw_blend_ch(o & 255u, c & 255u, fr.wa, fr.wb, fr.gamma) |
                 (draw_blend_ch((o >> 8) & 255u, (c >> 8) & 255u, fr.wa, fr.wb, fr.gamma) << 8) |
                 (draw_blend_ch((o >> 16) & 255u, (c >> 16) & 255u, fr.wa, fr.wb, fr.gamma) << 16);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kDrawRows; ++k) {
    if (!in[k]) continue;
    const int y = ty0 + wave + k * (kDrawThreads / kDrawTileW);
    uint8_t* p = fr.dst + ((int64_t)y * fr.w + x) * 3;
    p[0] = (uint8_t)(cur[k] & 255u);
    p[1] = (uint8_t)((cur[k] >> 8) & 255u);
    p[2] = (uint8_t)((cur[k] >> 16) & 255u);
  }
}

// ---- host ----
struct DrawHost {
  std::vector<DrawFrame> frames;  // src / dst still unset
  std::vector<DrawBox> boxes;
  std::vector<DrawRec> recs;
  int64_t tiles = 0;
};

// Validates the lists of n frames (frame f is hw[2f] x hw[2f + 1]) and lays the records out; makes
// no HIP call.
int draw_pack(const char* who, int32_t n, const int32_t* hw, const int32_t* prim_offsets, const op_draw_prim* prims,
              DrawHost* out) {
  if (!prim_offsets) return invalid(who, "null prim_offsets");
  int64_t prev = 0;
  for (int f = 0; f <= n; ++f) {
    if ((f == 0 && prim_offsets[f] != 0) || prim_offsets[f] < prev)
      return invalid(who, "prim_offsets: entry " + std::to_string(f) + " must start at 0 and never decrease");
    prev = prim_offsets[f];
  }
  if (prim_offsets[n] > 0 && !prims) return invalid(who, "null prims");
  auto coord = [](double v) { return std::isfinite(v) && std::fabs(v) <= kDrawMaxCoord; };
  out->frames.resize(n);
  out->recs.reserve((size_t)prim_offsets[n]);
  for (int f = 0; f < n; ++f) {
    DrawFrame& fr = out->frames[f];
    memset(&fr, 0, sizeof(fr));
    fr.h = hw[2 * f];
    fr.w = hw[2 * f + 1];
    fr.p0 = (int32_t)out->recs.size();
    fr.pb = -1;
    for (int i = prim_offsets[f]; i < prim_offsets[f + 1]; ++i) {
      const op_draw_prim& p = prims[i];
      const std::string at = "prims: primitive " + std::to_string(i) + ": ";
      DrawRec r;
      DrawBox b;
      memset(&r, 0, sizeof(r));
      if (p.kind == OP_DRAW_BLEND) {
        if (fr.pb >= 0) return invalid(who, at + "kind: more than one BLEND in the list of frame " + std::to_string(f));
        if (!std::isfinite(p.wa) || !std::isfinite(p.wb) || !std::isfinite(p.gamma))
          return invalid(who, at + "wa, wb, gamma: a blend weight that is not finite");
        fr.pb = (int32_t)out->recs.size();
        fr.blend = 1;
        fr.wa = p.wa;
        fr.wb = p.wb;
        fr.gamma = p.gamma;
        continue;
      }
      if (p.kind == OP_DRAW_LINE) {
        if (!coord(p.x0) || !coord(p.y0) || !coord(p.x1) || !coord(p.y1))
          return invalid(who, at + "x0, y0, x1, y1: a coordinate that is not finite or above 32768 in magnitude");
        if (!(p.thickness > 0.0) || !(p.thickness <= kDrawMaxCoord))
          return invalid(who, at + "thickness must be in (0, 32768]");
        const double rr = p.thickness / 2.0;
        r.x0 = p.x0;
        r.y0 = p.y0;
        r.dx = p.x1 - p.x0;
        r.dy = p.y1 - p.y0;
        r.n2 = r.dx * r.dx + r.dy * r.dy;
        r.r2 = rr * rr;
        r.cull2 = (rr + kDrawReach) * (rr + kDrawReach);
        b.lx = (int32_t)std::floor((p.x0 < p.x1 ? p.x0 : p.x1) - rr);
        b.hx = (int32_t)std::ceil((p.x0 > p.x1 ? p.x0 : p.x1) + rr);
        b.ly = (int32_t)std::floor((p.y0 < p.y1 ? p.y0 : p.y1) - rr);
        b.hy = (int32_t)std::ceil((p.y0 > p.y1 ? p.y0 : p.y1) + rr);
        r.col = 0u;
      } else if (p.kind == OP_DRAW_DISC) {
        if (!coord(p.x0) || !coord(p.y0) || p.x0 != std::floor(p.x0) || p.y0 != std::floor(p.y0))
          return invalid(who, at + "x0, y0: a disc centre that is not a whole number of at most 32768 in magnitude");
        if (p.radius < 0 || p.radius > kDrawMaxRadius) return invalid(who, at + "radius must be in 0 .. 1024");
        const int32_t cx = (int32_t)p.x0, cy = (int32_t)p.y0;
        b.lx = cx - p.radius;
        b.hx = cx + p.radius;
        b.ly = cy - p.radius;
        b.hy = cy + p.radius;
        r.col = kDrawDiscBit;
      } else {
        return invalid(who, at + "unknown kind " + std::to_string(p.kind));
      }
      r.col |= (uint32_t)p.bgr[0] | ((uint32_t)p.bgr[1] << 8) | ((uint32_t)p.bgr[2] << 16);
      out->boxes.push_back(b);
      out->recs.push_back(r);
    }
    fr.p1 = (int32_t)out->recs.size();
    if (fr.pb < 0) fr.pb = fr.p1;
    fr.tiles_x = (fr.w + kDrawTileW - 1) / kDrawTileW;
    if (out->tiles > INT32_MAX) return invalid(who, "more than 2^31 - 1 pixel tiles in the batch");
    fr.tile0 = (int32_t)out->tiles;
    out->tiles += (int64_t)fr.tiles_x * ((fr.h + kDrawTileH - 1) / kDrawTileH);
  }
  if (out->tiles > INT32_MAX) return invalid(who, "more than 2^31 - 1 pixel tiles in the batch");
  return OP_OK;
}

LastMs g_draw_last;

// The device tables of dh in the job's buffers
DrawArgs draw_alloc(Job& job, const DrawHost& dh) {
  DrawArgs a;
  a.frames = (const DrawFrame*)job.alloc(dh.frames.size() * sizeof(DrawFrame));
  a.boxes = (const DrawBox*)job.alloc(dh.boxes.size() * sizeof(DrawBox));
  a.recs = (const DrawRec*)job.alloc(dh.recs.size() * sizeof(DrawRec));
  a.n = (int32_t)dh.frames.size();
  return a;
}

// Uploads dh (its frames' src / dst set) and queues draw_tiles; ends the job's timing
void draw_run(Job& job, const DrawHost& dh, const DrawArgs& a) {
  job.upload((void*)a.frames, dh.frames.data(), dh.frames.size() * sizeof(DrawFrame));
  job.upload((void*)a.boxes, dh.boxes.data(), dh.boxes.size() * sizeof(DrawBox));
  job.upload((void*)a.recs, dh.recs.data(), dh.recs.size() * sizeof(DrawRec));
  if (job.ok()) {
    hipLaunchKernelGGL(draw_tiles, dim3((unsigned)dh.tiles), dim3(kDrawThreads), 0, job.stream(), a);
    job.check(hipGetLastError(), "draw_tiles");
  }
  job.end();
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_draw(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
                       const int32_t* hw, const int32_t* prim_offsets, const op_draw_prim* prims,
                       uint8_t* const* out) {
  const char* who = "op_draw";
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  RC(check_frames(who, n, bgr, row_stride, hw, out));
  DrawHost dh;
  RC(draw_pack(who, n, hw, prim_offsets, prims, &dh));
  RC(use_device(who, device));
  std::vector<int64_t> off(n + 1, 0);  // source and destination frames share one layout: rows of 3 w bytes
  for (int f = 0; f < n; ++f) off[f + 1] = off[f] + pad16((int64_t)dh.frames[f].h * dh.frames[f].w * 3);
  Job job(who, nullptr);
  const DrawArgs a = draw_alloc(job, dh);
  uint8_t* src = (uint8_t*)job.alloc((size_t)off[n]);
  uint8_t* dst = (uint8_t*)job.alloc((size_t)off[n]);
  job.begin();
  for (int f = 0; f < n && job.ok(); ++f) {
    DrawFrame& fr = dh.frames[f];
    fr.src = src + off[f];
    fr.dst = dst + off[f];
    fr.src_stride = (int64_t)fr.w * 3;
    job.upload2d((void*)fr.src, (size_t)fr.w * 3, bgr[f], (size_t)row_stride[f], (size_t)fr.w * 3, (size_t)fr.h,
                 "frame upload");
  }
  draw_run(job, dh, a);
  job.finish("kernel");
  for (int f = 0; f < n; ++f) job.download(out[f], dh.frames[f].dst, (size_t)dh.frames[f].h * dh.frames[f].w * 3);
  if (job.ok()) g_draw_last.done(device, job.ms());
  return job.status();
}

extern "C" int op_draw_staged(op_ctx* c, int32_t first, int32_t n, const int32_t* prim_offsets,
                              const op_draw_prim* prims, uint8_t* out) {
  const char* who = "op_draw_staged";
  if (!c) return invalid(who, "null context");
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  if (!out) return invalid(who, "null out");
  RC(staged_range(c, who, first, n));
  if (c->st_h > kDrawMaxSide || c->st_w > kDrawMaxSide) return invalid(who, "staged frames above 16384 in h or w");
  std::vector<int32_t> hw((size_t)n * 2);
  for (int f = 0; f < n; ++f) {
    hw[2 * f] = c->st_h;
    hw[2 * f + 1] = c->st_w;
  }
  DrawHost dh;
  RC(draw_pack(who, n, hw.data(), prim_offsets, prims, &dh));
  RC(check_ctx(c, false));
  const size_t fbytes = (size_t)c->st_h * c->st_w * 3;
  Job job(who, c->stream);  // everything is ordered on the context stream, behind a queued run
  const DrawArgs a = draw_alloc(job, dh);
  uint8_t* dst = (uint8_t*)job.alloc(fbytes * n);
  for (int f = 0; f < n && job.ok(); ++f) {
    DrawFrame& fr = dh.frames[f];
    fr.src = c->d_frames + (size_t)(first + f) * fbytes;  // read in place
    fr.dst = dst + (size_t)f * fbytes;
    fr.src_stride = (int64_t)c->st_w * 3;
  }
  job.begin();
  draw_run(job, dh, a);
  job.download(out, dst, fbytes * n);
  if (job.finish("kernel") == OP_OK) g_draw_last.done(c->device, job.ms());
  return job.status();
}

extern "C" int op_staged_info(op_ctx* c, int32_t* n, int32_t* h, int32_t* w) {
  if (!c) return invalid("op_staged_info", "null context");
  if (!n || !h || !w) return invalid("op_staged_info", "null output");
  const bool any = c->st_n > 0;
  *n = any ? c->st_n : 0;
  *h = any ? c->st_h : 0;
  *w = any ? c->st_w : 0;
  return OP_OK;
}

extern "C" int op_draw_last_ms(int32_t device, double* ms) {
  return g_draw_last.get("op_draw_last_ms", "op_draw or op_draw_staged", device, ms);
}
