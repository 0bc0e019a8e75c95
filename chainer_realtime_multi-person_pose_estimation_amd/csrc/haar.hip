// Faces from a Haar cascade on the device (haar.py is the statement, and the kernels
// equal it bit for bit: every float operation is written as its rounded intrinsic).
//
// A call works through its frames in chunks bounded by a byte budget.  Per chunk, whatever mix of
// sizes it holds (blockIdx.y = the frame or the layer, blockIdx.x runs over the largest one's work):
//   haar_grey      BGR -> grey, one thread per pixel (grey input is copied straight into place)
//   haar_pyramid   every layer of every frame: one thread per layer pixel, the four taps of the
//                  integer bilinear resize (the 8.8 horizontal values never leave registers)
//   haar_rows      one wave per layer row: shuffle scans over 64 pixels with the carry in a register,
//                  sum and sqsum from one read of the pixels
//   haar_cols      64 columns per workgroup, the rows split over its four waves: a wave totals its
//                  rows, the totals meet in LDS, a second pass writes the running sums
//   haar_dense     one lane per position of the step grid: setWindow and stage 0 -> map = -1 | 0 | 1
//   haar_resolve   one wave per grid row: OpenCV's skip (a valid window that fails stage 0 hides its
//                  right neighbour) is a two-state automaton; a ballot of the "hides" bits gives every
//                  lane its state from the nearest reset below it, the carry crosses 64-position
//                  pieces in a register.  Hidden positions become -2, visited stage-0 survivors are
//                  compacted (ballot + one atomic per wave) into a list of map offsets
//   haar_list      a few launches over the compacted lists (stages 1-3, 4-8, 9-14, the rest): a lane
//                  per survivor, the stump tables read wave-uniformly (scalar loads), survivors
//                  compacted again between launches so the long late stages run on full waves; the
//                  last one appends to its frame's candidate list (a cap per frame, the count goes on)
// The candidates are map offsets: sorted on the host they are in (layer, y, x) order.  Grouping is
// host code (haar_host.hpp).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "haar_host.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kHaarThreads = 256;
constexpr int kHaarWaves = kHaarThreads / 64;
constexpr int kHaarChunkFrames = 1000;                  // layers of a chunk stay below gridDim.y's 65535
constexpr int64_t kHaarChunkBytes = (int64_t)1 << 30;   // pyramids, maps and lists of one chunk
constexpr int kHaarListBlocks = 2048;                   // the list kernels stride over their input
constexpr int kHaarDefaultCandidates = 4096;
constexpr int kHaarMaxCandidates = 1 << 20;
constexpr int kHaarMaxFrames = 1 << 20;
constexpr int kHaarSegments[] = {1, 4, 9, 15};  // first stages of the list launches

struct HaarStump {  // 80 bytes, read wave-uniformly
  int32_t r[3][4];
  float w[3];
  float thr, left, right;
  int32_t pad[2];
};

struct HaarCascade {  // a kernel argument
  const HaarStump* stumps;
  const int32_t* first;
  const float* sthr;
  int32_t win_w, win_h, n_stages;
};

struct HaarFrame {
  const uint8_t* src;  // device pixels (BGR); null: the grey image was uploaded in place
  int64_t stride;
  int64_t grey_off;
  int32_t h, w;
};

struct HaarLayer {
  int64_t grey_off, pix_off, int_off;
  double sx, sy;     // source / layer size
  uint32_t map_off;  // the layer's first byte in the chunk's result map
  int32_t sh, sw, lh, lw;
  int32_t gy, gx, step;
  int32_t frame;     // within the chunk
  float sc;
  int32_t pad;
};

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(kHaarThreads) void haar_grey(const HaarFrame* __restrict__ F, uint8_t* __restrict__ grey) {
  const HaarFrame f = F[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * kHaarThreads + threadIdx.x;
  if (!f.src || i >= (int64_t)f.h * f.w) return;
  const int y = (int)(i / f.w), x = (int)(i - (int64_t)y * f.w);
  const uint8_t* p = f.src + y * f.stride + 3 * x;
  grey[f.grey_off + i] = (uint8_t)((1868u * p[0] + 9617u * p[1] + 4899u * p[2] + 8192u) >> 14);
}

// f = (d + 0.5) s - 0.5; the cell, its neighbour (both clamped) and the upper weight rint(frac 256)
__device__ __forceinline__ void haar_axis(int d, double s, int n, int* i0, int* i1, uint32_t* a) {
  const double f = __dsub_rn(__dmul_rn((double)d + 0.5, s), 0.5);
  const double c = floor(f);
  *a = (uint32_t)(int)rint(__dmul_rn(__dsub_rn(f, c), 256.0));
  const int ci = (int)c;
  *i0 = min(max(ci, 0), n - 1);
  *i1 = min(max(ci + 1, 0), n - 1);
}

__global__ __launch_bounds__(kHaarThreads) void haar_pyramid(const HaarLayer* __restrict__ L,
                                                            const uint8_t* __restrict__ grey,
                                                            uint8_t* __restrict__ pix) {
  const HaarLayer l = L[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * kHaarThreads + threadIdx.x;
  if (i >= (int64_t)l.lh * l.lw) return;
  const int dy = (int)(i / l.lw), dx = (int)(i - (int64_t)dy * l.lw);
  int x0, x1, y0, y1;
  uint32_t ax, ay;
  haar_axis(dx, l.sx, l.sw, &x0, &x1, &ax);
  haar_axis(dy, l.sy, l.sh, &y0, &y1, &ay);
  const uint8_t* r0 = grey + l.grey_off + (int64_t)y0 * l.sw;
  const uint8_t* r1 = grey + l.grey_off + (int64_t)y1 * l.sw;
  const uint32_t h0 = r0[x0] * (256u - ax) + r0[x1] * ax;  // 8.8, at most 255 * 256
  const uint32_t h1 = r1[x0] * (256u - ax) + r1[x1] * ax;
  pix[l.pix_off + i] = (uint8_t)((h0 * (256u - ay) + h1 * ay + 32768u) >> 16);
}

__global__ __launch_bounds__(kHaarThreads) void haar_rows(const HaarLayer* __restrict__ L,
                                                         const uint8_t* __restrict__ pix, uint32_t* __restrict__ sum,
                                                         uint32_t* __restrict__ sq) {
  const HaarLayer l = L[blockIdx.y];
  const int lane = threadIdx.x & 63, y = blockIdx.x * kHaarWaves + (threadIdx.x >> 6);
  if (y >= l.lh) return;  // a whole wave
  const int pitch = l.lw + 1;
  uint32_t* S = sum + l.int_off;
  uint32_t* Q = sq + l.int_off;
  if (y == 0)
    for (int x = lane; x < pitch; x += 64) S[x] = Q[x] = 0;
  const uint8_t* p = pix + l.pix_off + (int64_t)y * l.lw;
  uint32_t* Sr = S + (int64_t)(y + 1) * pitch;
  uint32_t* Qr = Q + (int64_t)(y + 1) * pitch;
  if (lane == 0) Sr[0] = Qr[0] = 0;
  uint32_t cs = 0, cq = 0;
  for (int x0 = 0; x0 < l.lw; x0 += 64) {
    const int x = x0 + lane;
    const uint32_t v = x < l.lw ? p[x] : 0u;
    uint32_t s = v, q = v * v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ts = __shfl_up(s, d), tq = __shfl_up(q, d);
      if (lane >= d) {
        s += ts;
        q += tq;
      }
    }
    if (x < l.lw) {
      Sr[x + 1] = cs + s;
      Qr[x + 1] = cq + q;
    }
    cs += __shfl(s, 63);
    cq += __shfl(q, 63);
  }
}

// blockIdx.z: 0 sum, 1 sqsum (both modulo 2^32)
__global__ __launch_bounds__(kHaarThreads) void haar_cols(const HaarLayer* __restrict__ L, uint32_t* __restrict__ sum,
                                                         uint32_t* __restrict__ sq) {
  __shared__ uint32_t tot[kHaarWaves][64];
  const HaarLayer l = L[blockIdx.y];
  if ((int)blockIdx.x * 64 >= l.lw) return;  // the whole workgroup
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane + 1, pitch = l.lw + 1;
  uint32_t* A = (blockIdx.z ? sq : sum) + l.int_off;
  const int rows = (l.lh + kHaarWaves - 1) / kHaarWaves;
  const int r0 = 1 + w * rows, r1 = min(r0 + rows, l.lh + 1);
  const bool on = c <= l.lw;
  uint32_t t = 0;
  if (on)
    for (int r = r0; r < r1; ++r) t += A[(int64_t)r * pitch + c];
  tot[w][lane] = t;
  __syncthreads();
  uint32_t run = 0;
  for (int k = 0; k < w; ++k) run += tot[k][lane];
  if (on)
    for (int r = r0; r < r1; ++r) {
      run += A[(int64_t)r * pitch + c];
      A[(int64_t)r * pitch + c] = run;
    }
}

// setWindow at (x, y): the window's corner in `sum`, 1 / sqrt(area sqsum - sum^2) as f32, and whether
// the window is looked at
__device__ __forceinline__ bool haar_window(const HaarCascade& C, int64_t int_off, int pitch, const uint32_t* sum,
                                            const uint32_t* sq, int x, int y, const int32_t** corner, float* vnf) {
  const int64_t o = int_off + (int64_t)y * pitch + x;
  const uint32_t* S = sum + o;
  const uint32_t* Q = sq + o;
  *corner = (const int32_t*)S;
  const int nw = C.win_w - 2, nh = C.win_h - 2;
  const int a = pitch + 1, b = a + nw, c = (1 + nh) * pitch + 1, d = c + nw;
  const int32_t vs = (int32_t)(S[a] - S[b] - S[c] + S[d]);
  const uint32_t vq = Q[a] - Q[b] - Q[c] + Q[d];
  const double area = (double)(nw * nh);
  const double nf = __dsub_rn(__dmul_rn(area, (double)vq), __dmul_rn((double)vs, (double)vs));
  *vnf = 1.0f;
  if (!(nf > 0.0)) return false;
  *vnf = (float)__ddiv_rn(1.0, __dsqrt_rn(nf));
  return __fmul_rn((float)(nw * nh), *vnf) < 0.1f;
}

__device__ __forceinline__ float haar_rect(const int32_t* S, int pitch, const int32_t* r) {
  const int p0 = r[1] * pitch + r[0], p2 = p0 + r[3] * pitch;
  const uint32_t v = (uint32_t)S[p0] - (uint32_t)S[p0 + r[2]] - (uint32_t)S[p2] + (uint32_t)S[p2 + r[2]];
  return (float)(int32_t)v;
}

// stage k: a float32 running sum over its stumps in file order; fails below the stage threshold
__device__ __forceinline__ bool haar_stage(const HaarCascade& C, int k, const int32_t* S, int pitch, float vnf) {
  float total = 0.0f;
  const int j1 = C.first[k + 1];
  for (int j = C.first[k]; j < j1; ++j) {
    const HaarStump& t = C.stumps[j];
    float v = __fadd_rn(__fmul_rn(t.w[0], haar_rect(S, pitch, t.r[0])), __fmul_rn(t.w[1], haar_rect(S, pitch, t.r[1])));
    if (t.w[2] != 0.0f) v = __fadd_rn(v, __fmul_rn(t.w[2], haar_rect(S, pitch, t.r[2])));
    v = __fmul_rn(v, vnf);
    total = __fadd_rn(total, v < t.thr ? t.left : t.right);
  }
  return !(total < C.sthr[k]);
}

__global__ __launch_bounds__(kHaarThreads) void haar_dense(HaarCascade C, const HaarLayer* __restrict__ L,
                                                          const uint32_t* __restrict__ sum,
                                                          const uint32_t* __restrict__ sq, int8_t* __restrict__ map) {
  const HaarLayer l = L[blockIdx.y];
  const int64_t p = (int64_t)blockIdx.x * kHaarThreads + threadIdx.x;
  if (p >= (int64_t)l.gy * l.gx) return;
  const int iy = (int)(p / l.gx), ix = (int)(p - (int64_t)iy * l.gx);
  const int32_t* S;
  float vnf;
  int8_t res = -1;
  if (haar_window(C, l.int_off, l.lw + 1, sum, sq, ix * l.step, iy * l.step, &S, &vnf))
    res = haar_stage(C, 0, S, l.lw + 1, vnf) ? 1 : 0;
  map[(int64_t)l.map_off + p] = res;
}

// the lanes of `mask` append `value` to list[*count ..]: one atomic per wave
__device__ __forceinline__ void haar_append(bool put, uint32_t value, uint32_t* list, uint32_t* count, int lane) {
  const uint64_t mask = __ballot(put);
  if (!mask) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = __shfl(base, 0);
  if (put) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = value;
}

__global__ __launch_bounds__(kHaarThreads) void haar_resolve(const HaarLayer* __restrict__ L, int8_t* __restrict__ map,
                                                            uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  const HaarLayer l = L[blockIdx.y];
  const int lane = threadIdx.x & 63, iy = blockIdx.x * kHaarWaves + (threadIdx.x >> 6);
  if (iy >= l.gy) return;  // a whole wave
  const int64_t row_off = (int64_t)l.map_off + (int64_t)iy * l.gx;
  int8_t* row = map + row_off;
  bool base = true;  // the row's first position is looked at
  for (int x0 = 0; x0 < l.gx; x0 += 64) {
    const int ix = x0 + lane;
    const bool in = ix < l.gx;
    const int m = in ? (int)row[ix] : -1;
    const uint64_t hides = __ballot(m == 0);  // if looked at: valid and failed stage 0
    // looked at = 1 right of a position that does not hide, and toggles across each one that does
    const uint64_t resets = ~hides;
    const uint64_t below = resets & ((1ull << lane) - 1ull);
    const bool vis = below ? (((lane - 1 - (63 - __clzll((long long)below))) & 1) == 0) : (base != ((lane & 1) != 0));
    if (resets) base = (((63 - (63 - __clzll((long long)resets))) & 1) == 0);  // the state at lane 64
    if (in && !vis) row[ix] = -2;
    haar_append(in && vis && m == 1, (uint32_t)(row_off + ix), list, count, lane);
  }
}

__global__ __launch_bounds__(kHaarThreads) void haar_list(HaarCascade C, const HaarLayer* __restrict__ L, int nl,
                                                         const uint32_t* __restrict__ sum,
                                                         const uint32_t* __restrict__ sq, int8_t* __restrict__ map,
                                                         const uint32_t* __restrict__ in,
                                                         const uint32_t* __restrict__ in_count, uint32_t* __restrict__ out,
                                                         uint32_t* __restrict__ out_count, int k0, int k1, int last,
                                                         uint32_t* __restrict__ cand, uint32_t* __restrict__ cand_count,
                                                         int cand_cap) {
  const uint32_t n = *in_count;
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * kHaarThreads + threadIdx.x) >> 6;
  const uint64_t waves = (uint64_t)gridDim.x * kHaarWaves;
  for (uint64_t at = wave * 64; at < n; at += waves * 64) {  // wave-uniform
    const bool on = at + lane < n;
    bool alive = on;
    uint32_t off = 0;
    const int32_t* S = nullptr;
    int pitch = 0, frame = 0;
    float vnf = 1.0f;
    if (on) {
      off = in[at + lane];
      int lo = 0, hi = nl - 1;  // the last layer whose map starts at or below `off` (empty ones lie before it)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L[mid].map_off <= off)
          lo = mid;
        else
          hi = mid - 1;
      }
      const int gx = L[lo].gx, step = L[lo].step;
      const uint32_t p = off - L[lo].map_off;
      const int iy = (int)(p / (uint32_t)gx), ix = (int)(p - (uint32_t)iy * (uint32_t)gx);
      pitch = L[lo].lw + 1;
      frame = L[lo].frame;
      haar_window(C, L[lo].int_off, pitch, sum, sq, ix * step, iy * step, &S, &vnf);
    }
    for (int k = k0; k < k1; ++k) {
      if (!__ballot(alive)) break;
      if (alive && !haar_stage(C, k, S, pitch, vnf)) {
        alive = false;
        map[off] = (int8_t)k;
      }
    }
    if (last) {
      if (alive) {
        map[off] = (int8_t)C.n_stages;
        const uint32_t i = atomicAdd(cand_count + frame, 1u);
        if (i < (uint32_t)cand_cap) cand[(int64_t)frame * cand_cap + i] = off;
      }
    } else {
      haar_append(alive, off, out, out_count, lane);
    }
  }
}

// ---------------------------------------------------------------- host
struct HaarSrc {
  const uint8_t* host;  // or
  const uint8_t* dev;
  int32_t h, w, channels;
  int64_t stride;
};

struct HaarPlanLayer {
  haar::Scale s;
  int32_t gy, gx, step;
};

struct HaarProbe {  // op_haar_probe's destinations
  uint8_t* pixels;
  int32_t* sum;
  uint32_t* sqsum;
  int8_t* map;
};

struct HaarTimes {
  LastMs dev;
  double part[kMaxDevices][OP_HAAR_TIMES] = {};
} g_haar_last;

const char* kHaarRan = "op_haar_detect or op_haar_candidates or op_haar_detect_staged or op_haar_probe";

int grid_len(int extent, int step) { return extent > 0 ? (extent + step - 1) / step : 0; }

int check_params(const char* who, const op_haar_params* p) {
  if (!p) return invalid(who, "null params");
  if (!std::isfinite(p->scale_factor) || p->scale_factor < 1.01) return invalid(who, "scale_factor: must be finite and >= 1.01");
  if (p->min_w < 1 || p->min_h < 1) return invalid(who, "min_size: must be positive");
  if (p->has_max && (p->max_w < 1 || p->max_h < 1)) return invalid(who, "max_size: must be positive");
  if (p->max_candidates < 0 || p->max_candidates > kHaarMaxCandidates) return invalid(who, "max_candidates: must be in 0 .. 1048576");
  return OP_OK;
}

int check_frame(const char* who, int f, const uint8_t* img, int h, int w, int64_t stride, int channels) {
  const std::string at = "frame " + std::to_string(f);
  if (h < 1 || h > haar::kMaxSide || w < 1 || w > haar::kMaxSide) return invalid(who, "hw: " + at + ": h, w must be in 1 .. 16384");
  if (channels != 1 && channels != 3) return invalid(who, "channels: " + at + ": must be 1 (grey) or 3 (BGR)");
  if (!img) return invalid(who, "bgr: " + at + ": null image");
  if (stride < (int64_t)w * channels) return invalid(who, "row_stride: " + at + ": fewer than w channels bytes per row");
  return OP_OK;
}

}  // namespace
}  // namespace op

struct op_haar {
  int32_t device = 0;
  int32_t win_w = 0, win_h = 0, n_stages = 0, n_stumps = 0;
  op::HaarStump* d_stumps = nullptr;
  int32_t* d_first = nullptr;
  float* d_sthr = nullptr;
};

namespace op {
namespace {

int plan_frame(const char* who, const op_haar* H, int f, int h, int w, const op_haar_params& p,
               std::vector<HaarPlanLayer>* out) {
  std::vector<haar::Scale> sc;
  if (!haar::scales(h, w, H->win_w, H->win_h, p.scale_factor, p.min_w, p.min_h, p.has_max ? p.max_w : w,
                    p.has_max ? p.max_h : h, &sc))
    return invalid(who, "scale_factor: frame " + std::to_string(f) + " has more than 64 scales");
  out->clear();
  for (const haar::Scale& s : sc) {
    const int step = (double)s.sc >= 2.0 ? 1 : 2;
    out->push_back(HaarPlanLayer{s, grid_len(s.lh - H->win_h, step), grid_len(s.lw - H->win_w, step), step});
  }
  return OP_OK;
}

int64_t frame_bytes(const HaarSrc& s, const std::vector<HaarPlanLayer>& layers) {
  int64_t b = (int64_t)s.h * s.w * (s.host && s.channels == 3 ? 4 : 1);
  for (const HaarPlanLayer& l : layers)
    b += (int64_t)l.s.lh * l.s.lw + 8 * (int64_t)(l.s.lh + 1) * (l.s.lw + 1) + 9 * (int64_t)l.gy * l.gx;
  return b;
}

struct HaarChunk {
  int f0 = 0, nf = 0;
  std::vector<HaarFrame> frames;
  std::vector<HaarLayer> layers;
  int64_t raw = 0, grey = 0, pix = 0, integ = 0, map = 0;  // bytes / elements of the chunk's buffers
  int64_t max_fpx = 0, max_lpx = 0, max_pos = 0;
  int max_lh = 0, max_lw = 0, max_gy = 0;
  hipEvent_t ev[5] = {};
};

struct HaarEvents {  // the chunks' events outlive the job's wait
  std::vector<HaarChunk>* chunks;
  ~HaarEvents() {
    for (HaarChunk& c : *chunks)
      for (hipEvent_t e : c.ev)
        if (e) (void)hipEventDestroy(e);
  }
};

// Everything between validated arguments and sorted candidate keys.  cands[f]: frame f's candidates
// in (layer, y, x) order, or empty with need[f] > cap_c when the device list overflowed.
int haar_run(const char* who, const op_haar* H, hipStream_t stream, const std::vector<HaarSrc>& src,
             const std::vector<std::vector<HaarPlanLayer>>& plan, int cap_c, std::vector<std::vector<haar::Rect>>* cands,
             std::vector<int64_t>* need, const HaarProbe* probe) {
  const int n = (int)src.size();
  cands->assign((size_t)n, {});
  need->assign((size_t)n, 0);
  // chunks
  std::vector<HaarChunk> chunks;
  HaarEvents events{&chunks};
  int64_t total_layers = 0;
  for (int f = 0; f < n;) {
    HaarChunk c;
    c.f0 = f;
    int64_t bytes = 0;
    while (f < n && c.nf < kHaarChunkFrames) {
      const int64_t fb = frame_bytes(src[f], plan[f]);
      if (c.nf && bytes + fb > kHaarChunkBytes) break;
      bytes += fb;
      const HaarSrc& s = src[f];
      HaarFrame fr{};
      fr.h = s.h;
      fr.w = s.w;
      fr.grey_off = c.grey;
      c.grey += (int64_t)s.h * s.w;
      if (s.dev) {
        fr.src = s.dev;
        fr.stride = s.stride;
      } else if (s.channels == 3) {
        fr.src = (const uint8_t*)(intptr_t)c.raw;  // an offset until the buffer exists
        fr.stride = (int64_t)s.w * 3;
        c.raw += pad16((int64_t)s.h * s.w * 3);
      }
      if (!plan[f].empty()) c.max_fpx = std::max(c.max_fpx, (int64_t)s.h * s.w);
      for (const HaarPlanLayer& pl : plan[f]) {
        HaarLayer l{};
        l.grey_off = fr.grey_off;
        l.pix_off = c.pix;
        l.int_off = c.integ;
        l.sx = (double)s.w / (double)pl.s.lw;
        l.sy = (double)s.h / (double)pl.s.lh;
        l.map_off = (uint32_t)c.map;
        l.sh = s.h;
        l.sw = s.w;
        l.lh = pl.s.lh;
        l.lw = pl.s.lw;
        l.gy = pl.gy;
        l.gx = pl.gx;
        l.step = pl.step;
        l.frame = c.nf;
        l.sc = pl.s.sc;
        c.pix += (int64_t)l.lh * l.lw;
        c.integ += (int64_t)(l.lh + 1) * (l.lw + 1);
        c.map += (int64_t)l.gy * l.gx;
        c.max_lpx = std::max(c.max_lpx, (int64_t)l.lh * l.lw);
        c.max_pos = std::max(c.max_pos, (int64_t)l.gy * l.gx);
        c.max_lh = std::max(c.max_lh, l.lh);
        c.max_lw = std::max(c.max_lw, l.lw);
        c.max_gy = std::max(c.max_gy, l.gy);
        c.layers.push_back(l);
      }
      c.frames.push_back(fr);
      ++c.nf;
      ++f;
    }
    if (c.map >= ((int64_t)1 << 32)) return invalid(who, "a chunk's result map passes 2^32 positions");
    total_layers += (int64_t)c.layers.size();
    chunks.push_back(std::move(c));
  }
  if (!total_layers) return OP_OK;  // no frame holds a window: no device call
  HaarChunk big;  // the largest of every buffer
  int max_nf = 0;
  size_t max_nl = 0;
  for (const HaarChunk& c : chunks) {
    big.raw = std::max(big.raw, c.raw);
    big.grey = std::max(big.grey, c.grey);
    big.pix = std::max(big.pix, c.pix);
    big.integ = std::max(big.integ, c.integ);
    big.map = std::max(big.map, c.map);
    max_nf = std::max(max_nf, c.nf);
    max_nl = std::max(max_nl, c.layers.size());
  }
  std::vector<uint32_t> h_count((size_t)n, 0u), h_cand((size_t)n * cap_c, 0u);

  Job job(who, stream);
  uint8_t* d_raw = (uint8_t*)job.alloc((size_t)big.raw);
  uint8_t* d_grey = (uint8_t*)job.alloc((size_t)big.grey);
  uint8_t* d_pix = (uint8_t*)job.alloc((size_t)big.pix);
  uint32_t* d_sum = (uint32_t*)job.alloc((size_t)big.integ * 4);
  uint32_t* d_sq = (uint32_t*)job.alloc((size_t)big.integ * 4);
  int8_t* d_map = (int8_t*)job.alloc((size_t)std::max<int64_t>(big.map, 1));
  uint32_t* d_list[2] = {(uint32_t*)job.alloc((size_t)std::max<int64_t>(big.map, 1) * 4),
                         (uint32_t*)job.alloc((size_t)std::max<int64_t>(big.map, 1) * 4)};
  constexpr int kCounters = 16;  // the lists' lengths (one per list launch and one more), then the frames' candidate counts
  static_assert(sizeof(kHaarSegments) / sizeof(kHaarSegments[0]) + 1 <= kCounters, "a counter per list");
  uint32_t* d_count = (uint32_t*)job.alloc((size_t)(kCounters + max_nf) * 4);
  uint32_t* d_cand = (uint32_t*)job.alloc((size_t)max_nf * cap_c * 4);
  HaarFrame* d_frames = (HaarFrame*)job.alloc((size_t)max_nf * sizeof(HaarFrame));
  HaarLayer* d_layers = (HaarLayer*)job.alloc(max_nl * sizeof(HaarLayer));
  const HaarCascade C{H->d_stumps, H->d_first, H->d_sthr, H->win_w, H->win_h, H->n_stages};
  job.begin();
  for (HaarChunk& c : chunks) {
    if (c.layers.empty() || !job.ok()) continue;
    const int nl = (int)c.layers.size();
    bool any_bgr = false;
    for (int i = 0; i < c.nf; ++i) {
      const HaarSrc& s = src[c.f0 + i];
      HaarFrame& fr = c.frames[i];
      if (s.dev) {
        any_bgr = true;
      } else if (s.channels == 3) {
        uint8_t* dst = d_raw + (intptr_t)fr.src;
        job.upload2d(dst, (size_t)s.w * 3, s.host, (size_t)s.stride, (size_t)s.w * 3, (size_t)s.h, "frame upload");
        fr.src = dst;
        any_bgr = true;
      } else {
        job.upload2d(d_grey + fr.grey_off, (size_t)s.w, s.host, (size_t)s.stride, (size_t)s.w, (size_t)s.h, "frame upload");
      }
    }
    job.upload(d_frames, c.frames.data(), (size_t)c.nf * sizeof(HaarFrame), "table upload");
    job.upload(d_layers, c.layers.data(), (size_t)nl * sizeof(HaarLayer), "table upload");
    job.memset(d_count, 0, (size_t)(kCounters + c.nf) * 4);
    for (int i = 0; i < 5 && job.ok(); ++i) job.check(hipEventCreate(&c.ev[i]), "hipEventCreate");
    if (!job.ok()) break;
    hipStream_t st = job.stream();
    const auto blocks = [](int64_t v, int per) { return (unsigned)((v + per - 1) / per); };
    job.check(hipEventRecord(c.ev[0], st), "hipEventRecord");
    if (any_bgr) haar_grey<<<dim3(blocks(c.max_fpx, kHaarThreads), c.nf), kHaarThreads, 0, st>>>(d_frames, d_grey);
    job.check(hipEventRecord(c.ev[1], st), "hipEventRecord");
    haar_pyramid<<<dim3(blocks(c.max_lpx, kHaarThreads), nl), kHaarThreads, 0, st>>>(d_layers, d_grey, d_pix);
    job.check(hipEventRecord(c.ev[2], st), "hipEventRecord");
    haar_rows<<<dim3(blocks(c.max_lh, kHaarWaves), nl), kHaarThreads, 0, st>>>(d_layers, d_pix, d_sum, d_sq);
    haar_cols<<<dim3(blocks(c.max_lw, 64), nl, 2), kHaarThreads, 0, st>>>(d_layers, d_sum, d_sq);
    job.check(hipEventRecord(c.ev[3], st), "hipEventRecord");
    if (c.max_pos) {
      haar_dense<<<dim3(blocks(c.max_pos, kHaarThreads), nl), kHaarThreads, 0, st>>>(C, d_layers, d_sum, d_sq, d_map);
      haar_resolve<<<dim3(blocks(c.max_gy, kHaarWaves), nl), kHaarThreads, 0, st>>>(d_layers, d_map, d_list[0], d_count);
      constexpr int kSeg = (int)(sizeof(kHaarSegments) / sizeof(kHaarSegments[0]));
      for (int s = 0, li = 0; s < kSeg; ++s) {
        const int k0 = std::min(kHaarSegments[s], H->n_stages);
        const int k1 = s + 1 < kSeg ? std::min(kHaarSegments[s + 1], H->n_stages) : H->n_stages;
        const int last = k1 == H->n_stages;
        haar_list<<<kHaarListBlocks, kHaarThreads, 0, st>>>(C, d_layers, nl, d_sum, d_sq, d_map, d_list[li], d_count + s,
                                                           d_list[li ^ 1], d_count + s + 1, k0, k1, last, d_cand,
                                                           d_count + kCounters, cap_c);
        li ^= 1;
        if (last) break;
      }
    }
    job.check(hipEventRecord(c.ev[4], st), "hipEventRecord");
    job.check(hipGetLastError(), "kernel launch");
    job.download(h_count.data() + c.f0, d_count + kCounters, (size_t)c.nf * 4, "count download");
    job.download(h_cand.data() + (size_t)c.f0 * cap_c, d_cand, (size_t)c.nf * cap_c * 4, "candidate download");
    if (probe) {
      job.download(probe->pixels, d_pix, (size_t)c.pix, "probe download");
      job.download(probe->sum, d_sum, (size_t)c.integ * 4, "probe download");
      job.download(probe->sqsum, d_sq, (size_t)c.integ * 4, "probe download");
      job.download(probe->map, d_map, (size_t)c.map, "probe download");
    }
    // the next chunk reuses every buffer: on a stream its uploads queue behind these downloads
  }
  job.end();
  if (job.finish("kernel") != OP_OK) return job.status();
  double part[OP_HAAR_TIMES] = {job.ms(), 0, 0, 0, 0};
  for (const HaarChunk& c : chunks)
    for (int i = 0; i < 4 && c.ev[4]; ++i) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, c.ev[i], c.ev[i + 1]) == hipSuccess) part[i + 1] += ms;
    }
  {
    std::lock_guard<std::mutex> lock(g_haar_last.dev.mutex);
    if (H->device >= 0 && H->device < kMaxDevices) {
      g_haar_last.dev.ms[H->device] = part[0];
      g_haar_last.dev.ran[H->device] = true;
      for (int i = 0; i < OP_HAAR_TIMES; ++i) g_haar_last.part[H->device][i] = part[i];
    }
  }
  // keys -> rectangles
  for (const HaarChunk& c : chunks) {
    size_t l0 = 0;
    for (int i = 0; i < c.nf; ++i) {
      const int f = c.f0 + i;
      size_t l1 = l0;
      while (l1 < c.layers.size() && c.layers[l1].frame == i) ++l1;
      const uint32_t cnt = h_count[f];
      (*need)[f] = cnt;
      if (cnt <= (uint32_t)cap_c && cnt) {
        uint32_t* keys = h_cand.data() + (size_t)f * cap_c;
        std::sort(keys, keys + cnt);
        std::vector<haar::Rect>& out = (*cands)[f];
        out.reserve(cnt);
        size_t li = l0;
        for (uint32_t k = 0; k < cnt; ++k) {
          while (li + 1 < l1 && c.layers[li + 1].map_off <= keys[k]) ++li;
          const HaarLayer& l = c.layers[li];
          const uint32_t p = keys[k] - l.map_off;
          const int iy = (int)(p / (uint32_t)l.gx), ix = (int)(p % (uint32_t)l.gx);
          const double sc = (double)l.sc;
          out.push_back(haar::Rect{haar::rint_i(ix * l.step * sc), haar::rint_i(iy * l.step * sc),
                                   haar::rint_i(H->win_w * sc), haar::rint_i(H->win_h * sc)});
        }
      }
      l0 = l1;
    }
  }
  return OP_OK;
}

// the frames' outputs from their candidates: grouped (neighbours != null) or as they are
void haar_outputs(const op_haar_params& p, int cap_c, const std::vector<std::vector<haar::Rect>>& cands,
                  const std::vector<int64_t>& need, int32_t cap, int32_t* rects, int32_t* neighbours, int32_t* count,
                  int32_t* status) {
  std::vector<haar::Rect> grouped;
  std::vector<int32_t> neigh;
  for (size_t f = 0; f < cands.size(); ++f) {
    status[f] = OP_OK;
    if (need[f] > cap_c) {  // the device list overflowed: nothing of this frame is known
      status[f] = OP_ERR_CAPACITY;
      count[f] = (int32_t)need[f];
      continue;
    }
    const std::vector<haar::Rect>* r = &cands[f];
    if (neighbours) {
      haar::group_rectangles(cands[f], p.min_neighbors, 0.2, &grouped, &neigh);
      r = &grouped;
    }
    count[f] = (int32_t)r->size();
    if ((int64_t)r->size() > cap) {
      status[f] = OP_ERR_CAPACITY;
      continue;
    }
    for (size_t i = 0; i < r->size(); ++i) {
      int32_t* o = rects + ((int64_t)f * cap + (int64_t)i) * 4;
      o[0] = (*r)[i].x;
      o[1] = (*r)[i].y;
      o[2] = (*r)[i].w;
      o[3] = (*r)[i].h;
      if (neighbours) neighbours[(int64_t)f * cap + (int64_t)i] = neigh[i];
    }
  }
}

int haar_host_frames(const char* who, const op_haar* h, int32_t n, const uint8_t* const* bgr, const int32_t* hw,
                     const int64_t* row_stride, const int32_t* channels, const op_haar_params* params, int32_t cap,
                     int32_t* rects, int32_t* neighbours, bool grouped, int32_t* count, int32_t* status) {
  if (!h) return invalid(who, "null cascade");
  if (n < 0 || n > kHaarMaxFrames) return invalid(who, "n_frames must be in 0 .. 1048576");
  RC(check_params(who, params));
  if (cap < 0) return invalid(who, "cap: negative");
  if (n == 0) return OP_OK;
  if (!bgr) return invalid(who, "null bgr");
  if (!hw) return invalid(who, "null hw");
  if (!row_stride) return invalid(who, "null row_stride");
  if (!channels) return invalid(who, "null channels");
  if (!count || !status || (cap && !rects) || (grouped && cap && !neighbours)) return invalid(who, "null output");
  std::vector<HaarSrc> src((size_t)n);
  std::vector<std::vector<HaarPlanLayer>> plan((size_t)n);
  for (int f = 0; f < n; ++f) {
    RC(check_frame(who, f, bgr[f], hw[2 * f], hw[2 * f + 1], row_stride[f], channels[f]));
    src[f] = HaarSrc{bgr[f], nullptr, hw[2 * f], hw[2 * f + 1], channels[f], row_stride[f]};
    RC(plan_frame(who, h, f, src[f].h, src[f].w, *params, &plan[f]));
  }
  const int cap_c = params->max_candidates ? params->max_candidates : kHaarDefaultCandidates;
  std::vector<std::vector<haar::Rect>> cands;
  std::vector<int64_t> need;
  RC(use_device(who, h->device));
  RC(haar_run(who, h, nullptr, src, plan, cap_c, &cands, &need, nullptr));
  haar_outputs(*params, cap_c, cands, need, cap, rects, grouped ? neighbours : nullptr, count, status);
  return OP_OK;
}

int haar_staged(const char* who, const op_haar* h, op_ctx* c, int32_t first, int32_t n, const op_haar_params* params,
                int32_t cap, int32_t* rects, int32_t* neighbours, int32_t* count, int32_t* status) {
  if (!h) return invalid(who, "null cascade");
  if (!c) return invalid(who, "null context");
  RC(check_params(who, params));
  if (n < 1 || n > kHaarMaxFrames) return invalid(who, "n must be in 1 .. 1048576");
  if (cap < 0) return invalid(who, "cap: negative");
  if (!count || !status || (cap && (!rects || !neighbours))) return invalid(who, "null output");
  RC(staged_range(c, who, first, n));
  if (c->device != h->device) return invalid(who, "the cascade lives on another device than the context");
  if (c->st_h > haar::kMaxSide || c->st_w > haar::kMaxSide) return invalid(who, "staged frames above 16384 in h or w");
  RC(check_ctx(c, false));
  const size_t fbytes = (size_t)c->st_h * c->st_w * 3;
  std::vector<HaarSrc> src((size_t)n);
  std::vector<std::vector<HaarPlanLayer>> plan((size_t)n);
  for (int f = 0; f < n; ++f) {
    src[f] = HaarSrc{nullptr, c->d_frames + (size_t)(first + f) * fbytes, c->st_h, c->st_w, 3, (int64_t)c->st_w * 3};
    RC(plan_frame(who, h, f, src[f].h, src[f].w, *params, &plan[f]));
  }
  const int cap_c = params->max_candidates ? params->max_candidates : kHaarDefaultCandidates;
  std::vector<std::vector<haar::Rect>> cands;
  std::vector<int64_t> need;
  RC(haar_run(who, h, c->stream, src, plan, cap_c, &cands, &need, nullptr));
  haar_outputs(*params, cap_c, cands, need, cap, rects, neighbours, count, status);
  return OP_OK;
}

int haar_probe(const char* who, const op_haar* h, const uint8_t* bgr, int32_t fh, int32_t fw, int64_t row_stride,
               int32_t channels, const op_haar_params* params, int32_t* n_layers, int32_t* layer_hw, float* layer_scale,
               uint8_t* pixels, int32_t* sum, uint32_t* sqsum, int8_t* map, const int64_t* cap) {
  if (!h) return invalid(who, "null cascade");
  RC(check_params(who, params));
  if (!n_layers || !layer_hw || !layer_scale) return invalid(who, "null output");
  RC(check_frame(who, 0, bgr, fh, fw, row_stride, channels));
  std::vector<std::vector<HaarPlanLayer>> plan(1);
  RC(plan_frame(who, h, 0, fh, fw, *params, &plan[0]));
  *n_layers = (int32_t)plan[0].size();
  int64_t want[3] = {0, 0, 0};
  for (size_t i = 0; i < plan[0].size(); ++i) {
    const HaarPlanLayer& l = plan[0][i];
    layer_hw[2 * i] = l.s.lh;
    layer_hw[2 * i + 1] = l.s.lw;
    layer_scale[i] = l.s.sc;
    want[0] += (int64_t)l.s.lh * l.s.lw;
    want[1] += (int64_t)(l.s.lh + 1) * (l.s.lw + 1);
    want[2] += (int64_t)l.gy * l.gx;
  }
  if (!pixels) return OP_OK;
  if (!sum || !sqsum || !map || !cap) return invalid(who, "null output");
  if (cap[0] < want[0] || cap[1] < want[1] || cap[2] < want[2]) {
    set_error(std::string(who) + ": cap: the layers need " + std::to_string(want[0]) + " pixels, " + std::to_string(want[1]) +
              " integral elements and " + std::to_string(want[2]) + " map bytes");
    return OP_ERR_CAPACITY;
  }
  std::vector<HaarSrc> src{HaarSrc{bgr, nullptr, fh, fw, channels, row_stride}};
  const int cap_c = params->max_candidates ? params->max_candidates : kHaarDefaultCandidates;
  std::vector<std::vector<haar::Rect>> cands;
  std::vector<int64_t> need;
  const HaarProbe probe{pixels, sum, sqsum, map};
  RC(use_device(who, h->device));
  return haar_run(who, h, nullptr, src, plan, cap_c, &cands, &need, &probe);
}

int haar_create(const char* who, int32_t device, int32_t win_w, int32_t win_h, int32_t n_stages,
                const int32_t* stage_first, const float* stage_thr, int32_t n_stumps, const int32_t* rects,
                const float* weights, const float* thr, const float* left, const float* right, op_haar** out) {
  if (!out) return invalid(who, "null out");
  *out = nullptr;
  if (win_w < 3 || win_w > haar::kMaxWindow || win_h < 3 || win_h > haar::kMaxWindow)
    return invalid(who, "win_w, win_h: must be in 3 .. 64");
  if (n_stages < 1 || n_stages > 127) return invalid(who, "n_stages: must be in 1 .. 127");
  if (n_stumps < 1 || n_stumps > (1 << 20)) return invalid(who, "n_stumps: must be in 1 .. 1048576");
  if (!stage_first || !stage_thr || !rects || !weights || !thr || !left || !right) return invalid(who, "null table");
  if (stage_first[0] != 0 || stage_first[n_stages] != n_stumps) return invalid(who, "stage_first: must run from 0 to n_stumps");
  for (int s = 0; s < n_stages; ++s)
    if (stage_first[s + 1] <= stage_first[s]) return invalid(who, "stage_first: stage " + std::to_string(s) + " is empty");
  std::vector<HaarStump> stumps((size_t)n_stumps);
  for (int j = 0; j < n_stumps; ++j) {
    HaarStump& t = stumps[j];
    memset(&t, 0, sizeof(t));
    for (int k = 0; k < 3; ++k) {
      const int32_t* r = rects + ((size_t)j * 3 + k) * 4;
      t.w[k] = weights[(size_t)j * 3 + k];
      if (k == 2 && t.w[k] == 0.0f) continue;  // no third rect: never read
      if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0 || r[0] + (int64_t)r[2] > win_w || r[1] + (int64_t)r[3] > win_h)
        return invalid(who, "rects: stump " + std::to_string(j) + ": a rect lies outside the window");
      for (int q = 0; q < 4; ++q) t.r[k][q] = r[q];
    }
    t.thr = thr[j];
    t.left = left[j];
    t.right = right[j];
  }
  RC(use_device(who, device));
  op_haar* h = new op_haar();
  h->device = device;
  h->win_w = win_w;
  h->win_h = win_h;
  h->n_stages = n_stages;
  h->n_stumps = n_stumps;
  hipError_t e = hipMalloc((void**)&h->d_stumps, stumps.size() * sizeof(HaarStump));
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_first, (size_t)(n_stages + 1) * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_sthr, (size_t)n_stages * 4);
  if (e == hipSuccess) e = hipMemcpy(h->d_stumps, stumps.data(), stumps.size() * sizeof(HaarStump), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_first, stage_first, (size_t)(n_stages + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_sthr, stage_thr, (size_t)n_stages * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error(std::string(who) + ": table upload: " + hipGetErrorString(e));
    op_haar_destroy(h);
    return OP_ERR_HIP;
  }
  *out = h;
  return OP_OK;
}

// The host tables of a batch are sized by the frames: an allocation that fails comes back as a status,
// not as an exception through the C interface
template <class Fn>
int guarded(const char* who, Fn fn) {
  try {
    return fn(who);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory for the batch's tables");
    return OP_ERR_CAPACITY;
  }
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_haar_create(int32_t device, int32_t win_w, int32_t win_h, int32_t n_stages, const int32_t* stage_first,
                              const float* stage_thr, int32_t n_stumps, const int32_t* rects, const float* weights,
                              const float* thr, const float* left, const float* right, op_haar** out) {
  return guarded("op_haar_create", [&](const char* who) {
    return haar_create(who, device, win_w, win_h, n_stages, stage_first, stage_thr, n_stumps, rects, weights, thr, left, right, out);
  });
}

extern "C" int op_haar_destroy(op_haar* h) {
  if (!h) return OP_OK;
  if (hipSetDevice(h->device) == hipSuccess) {
    if (h->d_stumps) (void)hipFree(h->d_stumps);
    if (h->d_first) (void)hipFree(h->d_first);
    if (h->d_sthr) (void)hipFree(h->d_sthr);
  }
  delete h;
  return OP_OK;
}

extern "C" int op_haar_detect(const op_haar* h, int32_t n_frames, const uint8_t* const* bgr, const int32_t* hw,
                              const int64_t* row_stride, const int32_t* channels, const op_haar_params* params,
                              int32_t cap, int32_t* rects, int32_t* neighbours, int32_t* count, int32_t* status) {
  return guarded("op_haar_detect", [&](const char* who) {
    return haar_host_frames(who, h, n_frames, bgr, hw, row_stride, channels, params, cap, rects, neighbours, true, count, status);
  });
}

extern "C" int op_haar_candidates(const op_haar* h, int32_t n_frames, const uint8_t* const* bgr, const int32_t* hw,
                                  const int64_t* row_stride, const int32_t* channels, const op_haar_params* params,
                                  int32_t cap, int32_t* rects, int32_t* count, int32_t* status) {
  return guarded("op_haar_candidates", [&](const char* who) {
    return haar_host_frames(who, h, n_frames, bgr, hw, row_stride, channels, params, cap, rects, nullptr, false, count, status);
  });
}

extern "C" int op_haar_detect_staged(const op_haar* h, op_ctx* ctx, int32_t first, int32_t n, const op_haar_params* params,
                                     int32_t cap, int32_t* rects, int32_t* neighbours, int32_t* count, int32_t* status) {
  return guarded("op_haar_detect_staged", [&](const char* who) {
    return haar_staged(who, h, ctx, first, n, params, cap, rects, neighbours, count, status);
  });
}

extern "C" int op_haar_probe(const op_haar* h, const uint8_t* bgr, int32_t fh, int32_t fw, int64_t row_stride,
                             int32_t channels, const op_haar_params* params, int32_t* n_layers, int32_t* layer_hw,
                             float* layer_scale, uint8_t* pixels, int32_t* sum, uint32_t* sqsum, int8_t* map,
                             const int64_t* cap) {
  return guarded("op_haar_probe", [&](const char* who) {
    return haar_probe(who, h, bgr, fh, fw, row_stride, channels, params, n_layers, layer_hw, layer_scale, pixels, sum, sqsum,
                      map, cap);
  });
}

extern "C" int op_haar_last_ms(int32_t device, double* ms) {
  const char* who = "op_haar_last_ms";
  if (!ms) return invalid(who, "null ms");
  std::lock_guard<std::mutex> lock(g_haar_last.dev.mutex);
  RC(g_haar_last.dev.check(who, kHaarRan, device));
  for (int i = 0; i < OP_HAAR_TIMES; ++i) ms[i] = g_haar_last.part[device][i];
  return OP_OK;
}
