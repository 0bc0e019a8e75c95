// Ignore masks from COCO segmentations on the device (gen_ignore_mask.py:23-37 gen_masks,
// COCO.annToMask; masks.py is the statement, and the two agree bit for bit).
//
// Every part (one polygon or one uncompressed RLE) owns a toggle plane in HBM: h * w + 1 bits over
// the column-major pixel index x * h + y, followed by w + 1 column bits (bit c = the parity of the
// toggles that fall into column c, position h * w counting as column w).  Pixel i of the part is
// set iff the number of toggles <= i is odd.  Toggles are flipped with integer atomicXor only:
// the planes do not depend on scheduling, and equal positions cancel as the statement demands.
//
// Host (mask_pack): every argument is validated; per polygon edge the upsampled end points, the
// flip and the float64 slope (one IEEE division, as the statement's) and the prefix of the edges'
// point counts; the RLE counts are compacted; every image is cut into blocks of columns.
// Device, three kernels over the whole batch:
//   mask_toggles: one thread per point d >= 1 of an edge's 5x upsampled outline.  It finds its edge
//     in the prefix (binary search), computes the points d and d - 1 in closed form (__dmul_rn /
//     __dadd_rn: three roundings, no contraction) and flips a bit where the outline crosses a pixel
//     column's centre line.
//   mask_rle: one workgroup per RLE part scans the counts (256 at a time, carry between chunks)
//     and flips the bit at every running sum.
//   mask_fill: one workgroup per block of columns of one image walks the image's annotations in
//     order.  Per part the block's toggle words go to LDS and become fill words by prefix-XOR:
//     shift-XOR doubling inside a word, a carry across a thread's words, wave ballots across
//     threads, and the column bits before the block as the carry-in.  The parts of an annotation
//     are ORed, mask_all / mask_miss of the block are kept in LDS under the three role rules, and
//     the row-major u8 masks are written at the end (an annotation's own mask only when asked for).
// mask_pack and mask_launch (masks.hpp) are shared with maskview.hip, whose kernel reads the masks
// where mask_fill left them.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "masks.hpp"

namespace op {
namespace {

constexpr int kMaskMaxSide = 16384;
constexpr double kMaskMaxCoord = 65536.0;
constexpr int kMaskUp = 5;  // rleFrPoly's upsampling
constexpr int kFillThreads = 256;
constexpr int kFillWords = 2048;  // LDS words per bit array of a column block
constexpr int kFillMaxCols = 64;

struct MaskArgs {
  const MaskImage* images;
  const MaskAnn* anns;
  const MaskPart* parts;
  const MaskEdge* edges;
  const int32_t* edge_start;  // [n_edges + 1]: prefix of len
  const MaskRle* rles;
  const uint32_t* counts;
  const MaskBlock* blocks;
  uint32_t* planes;
  uint8_t* out_all;
  uint8_t* out_miss;
  uint8_t* out_ann;
  int32_t n_edges, total_points;
};

__device__ __forceinline__ int mask_floor_div5(int v) { return v >= 0 ? v / 5 : -((4 - v) / 5); }

// the point at parameter t of an edge: (u, v)
__device__ __forceinline__ void mask_point(const MaskEdge& e, int t, int* u, int* v) {
  const int minor = (int)__dadd_rn(__dadd_rn((double)(e.major ? e.ys : e.xs), __dmul_rn(e.s, (double)t)), 0.5);
  *u = e.major ? e.xs + t : minor;
  *v = e.major ? minor : e.ys + t;
}

__device__ __forceinline__ void mask_flip(uint32_t* plane, int tw, int pos, int col) {
  atomicXor(plane + (pos >> 5), 1u << (pos & 31));
  atomicXor(plane + tw + (col >> 5), 1u << (col & 31));
}

__global__ __launch_bounds__(256) void mask_toggles(MaskArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= a.total_points) return;
  int lo = 0, hi = a.n_edges;  // the edge with edge_start[lo] <= gid < edge_start[lo + 1] (no edge is empty)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.edge_start[mid] <= gid) lo = mid; else hi = mid;
  }
  const MaskEdge e = a.edges[lo];
  const int d = (int)(gid - a.edge_start[lo]) + 1;
  int u1, v1, u0, v0;
  mask_point(e, e.flip ? e.len - d : d, &u1, &v1);
  mask_point(e, e.flip ? e.len - d + 1 : d - 1, &u0, &v0);
  if (u1 == u0) return;
  const int xd = u1 < u0 ? u1 : u1 - 1;  // (xd + 0.5) / 5 - 0.5 is an integer iff xd = 5 x + 2
  if (xd < 2 || (xd - 2) % kMaskUp != 0) return;
  const int x = (xd - 2) / kMaskUp;
  if (x > e.w - 1) return;
  int y = mask_floor_div5(min(v1, v0) + 2);  // ceil((yd + 0.5) / 5 - 0.5) = floor((yd + 2) / 5)
  y = y < 0 ? 0 : (y > e.h ? e.h : y);
  mask_flip(a.planes + e.plane_off, e.tw, x * e.h + y, x + (y == e.h ? 1 : 0));
}

__global__ __launch_bounds__(256) void mask_rle(MaskArgs a) {
  __shared__ uint32_t s[256];
  const MaskRle r = a.rles[blockIdx.x];
  const int tid = threadIdx.x;
  uint32_t carry = 0;
  for (int start = 0; start < r.n; start += 256) {
    const int i = start + tid;
    s[tid] = i < r.n ? a.counts[r.data_off + i] : 0u;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const uint32_t t = tid >= off ? s[tid - off] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (i < r.n) {
      const uint32_t pos = carry + s[tid];  // <= h * w: the host checked the sum
      mask_flip(a.planes + r.plane_off, r.tw, (int)pos, (int)(pos / (uint32_t)r.h));
    }
    carry += s[255];
    __syncthreads();
  }
}

// the block's columns of one bit array (column-major from bit `base`) as row-major bytes
__device__ __forceinline__ void mask_store(const uint32_t* bits, uint8_t* out, int h, int w, int c0, int nc, int base,
                                           int tid) {
  const int ng = (nc + 3) >> 2;
  for (int i = tid; i < h * ng; i += kFillThreads) {
    const int y = i / ng, j0 = (i - y * ng) * 4;
    const int cnt = min(4, nc - j0);
    uint32_t px = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < cnt) {
        const int l = (c0 + j0 + q) * h + y - base;
        px |= ((bits[l >> 5] >> (l & 31)) & 1u) << (8 * q);
      }
    uint8_t* p = out + (int64_t)y * w + c0 + j0;
    if (cnt == 4 && ((uintptr_t)p & 3) == 0) {
      *(uint32_t*)p = px;
    } else {
      for (int q = 0; q < cnt; ++q) p[q] = (uint8_t)((px >> (8 * q)) & 1u);
    }
  }
}

__global__ __launch_bounds__(kFillThreads) void mask_fill(MaskArgs a) {
  __shared__ uint32_t cur[kFillWords], acc[kFillWords], all[kFillWords], miss[kFillWords];
  __shared__ unsigned long long sbal[2][kFillThreads / 64];
  const MaskBlock b = a.blocks[blockIdx.x];
  const MaskImage im = a.images[b.image];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B0 = b.c0 * im.h, B1 = (b.c0 + b.nc) * im.h;  // the block's bits [B0, B1)
  const int Wb = B0 >> 5, nW = ((B1 - 1) >> 5) - Wb + 1;  // <= kFillWords by the host's choice of nc
  const int K = (nW + kFillThreads - 1) / kFillThreads;
  const int k0 = min(tid * K, nW), k1 = min(k0 + K, nW);  // this thread's words in the scan
  for (int k = tid; k < nW; k += kFillThreads) all[k] = miss[k] = 0u;
  for (int ai = im.ann0; ai < im.ann1; ++ai) {
    const MaskAnn an = a.anns[ai];
    for (int k = tid; k < nW; k += kFillThreads) acc[k] = 0u;
    for (int pi = an.part0; pi < an.part1; ++pi) {
      const MaskPart pt = a.parts[pi];
      const uint32_t* plane = a.planes + pt.plane_off;
      // the parity of every toggle before bit B0: the column bits 0 .. c0 - 1
      const uint32_t* cols = plane + pt.tw;
      uint32_t pre = 0u;
      for (int k = tid; k < (b.c0 >> 5); k += kFillThreads) pre ^= cols[k];
      if (tid == 0 && (b.c0 & 31)) pre ^= cols[b.c0 >> 5] & ((1u << (b.c0 & 31)) - 1u);
      pre = (uint32_t)__popc(pre) & 1u;
      for (int k = tid; k < nW; k += kFillThreads) {
        uint32_t x = plane[Wb + k];
        if (k == 0) x &= ~((1u << (B0 & 31)) - 1u);  // the bits before B0 are in the carry-in already
        cur[k] = x;
      }
      __syncthreads();
      uint32_t par = 0u;  // the parity of this thread's words so far
      for (int k = k0; k < k1; ++k) {
        uint32_t x = cur[k];
        x ^= x << 1;
        x ^= x << 2;
        x ^= x << 4;
        x ^= x << 8;
        x ^= x << 16;
        if (par) x = ~x;
        cur[k] = x;
        par = x >> 31;
      }
      const unsigned long long bal_par = __ballot((int)par), bal_pre = __ballot((int)pre);
      if (lane == 0) {
        sbal[0][wave] = bal_par;
        sbal[1][wave] = bal_pre;
      }
      __syncthreads();
      uint32_t carry = 0u;
      for (int v = 0; v < kFillThreads / 64; ++v) {
        carry ^= (uint32_t)__popcll(sbal[1][v]);
        if (v < wave) carry ^= (uint32_t)__popcll(sbal[0][v]);
      }
      carry ^= (uint32_t)__popcll(sbal[0][wave] & ((1ull << lane) - 1ull));
      if (carry & 1u)
        for (int k = k0; k < k1; ++k) cur[k] = ~cur[k];
      __syncthreads();
      for (int k = tid; k < nW; k += kFillThreads) acc[k] |= cur[k];
    }
    for (int k = tid; k < nW; k += kFillThreads) {
      const uint32_t m = acc[k];
      if (an.role == OP_MASK_CROWD) miss[k] |= m & ~all[k];
      if (an.role == OP_MASK_MISS) miss[k] |= m;
      all[k] |= m;
    }
    if (an.out_off >= 0) {
      __syncthreads();
      mask_store(acc, a.out_ann + an.out_off, im.h, im.w, b.c0, b.nc, Wb * 32, tid);
      __syncthreads();
    }
  }
  __syncthreads();
  mask_store(all, a.out_all + im.out_off, im.h, im.w, b.c0, b.nc, Wb * 32, tid);
  mask_store(miss, a.out_miss + im.out_off, im.h, im.w, b.c0, b.nc, Wb * 32, tid);
}

}  // namespace

// ---- host ----
int mask_offsets(const char* who, const char* name, const int64_t* o64, const int32_t* o32, int64_t count) {
  if (!o64 && !o32) return invalid(who, std::string("null ") + name);
  int64_t prev = 0;
  for (int64_t i = 0; i <= count; ++i) {
    const int64_t v = o64 ? o64[i] : (int64_t)o32[i];
    if ((i == 0 && v != 0) || v < prev)
      return invalid(who, std::string(name) + ": entry " + std::to_string(i) + " must start at 0 and never decrease");
    prev = v;
  }
  return OP_OK;
}

int mask_pack(const char* who, int32_t n, const int32_t* hw, const int32_t* ann_offsets, const int32_t* ann_role,
              const int32_t* part_offsets, const int32_t* part_kind, const int64_t* data_offsets, const double* xy,
              const uint32_t* counts, uint8_t* const* out_ann, uint8_t* const* ann_frames, MaskHost* out) {
  if (n < 1 || n > (1 << 20)) return invalid(who, "n must be in 1 .. 1048576");
  if (!hw) return invalid(who, "null hw");
  for (int f = 0; f < n; ++f)
    if (hw[2 * f] < 1 || hw[2 * f] > kMaskMaxSide || hw[2 * f + 1] < 1 || hw[2 * f + 1] > kMaskMaxSide)
      return invalid(who, "hw: image " + std::to_string(f) + ": h, w must be in 1 .. 16384");
  int rc = mask_offsets(who, "ann_offsets", nullptr, ann_offsets, n);
  if (rc) return rc;
  const int32_t A = ann_offsets[n];
  if (A > 0 && !ann_role) return invalid(who, "null ann_role");
  for (int a = 0; a < A; ++a)
    if (ann_role[a] != OP_MASK_KEEP && ann_role[a] != OP_MASK_MISS && ann_role[a] != OP_MASK_CROWD)
      return invalid(who, "ann_role: annotation " + std::to_string(a) + ": unknown role " + std::to_string(ann_role[a]));
  rc = mask_offsets(who, "part_offsets", nullptr, part_offsets, A);
  if (rc) return rc;
  const int32_t P = part_offsets[A];
  if (P > 0 && !part_kind) return invalid(who, "null part_kind");
  for (int p = 0; p < P; ++p)
    if (part_kind[p] != OP_MASK_POLYGON && part_kind[p] != OP_MASK_RLE)
      return invalid(who, "part_kind: part " + std::to_string(p) + ": unknown kind " + std::to_string(part_kind[p]));
  rc = mask_offsets(who, "data_offsets", data_offsets, nullptr, P);
  if (rc) return rc;
  int64_t points = 0;
  for (int f = 0; f < n; ++f) {
    const int64_t pixels = (int64_t)hw[2 * f] * hw[2 * f + 1];
    for (int p = part_offsets[ann_offsets[f]]; p < part_offsets[ann_offsets[f + 1]]; ++p) {
      const int64_t lo = data_offsets[p], len = data_offsets[p + 1] - lo;
      const std::string at = "part " + std::to_string(p) + ": ";
      if (part_kind[p] == OP_MASK_POLYGON) {
        if (!xy) return invalid(who, "null xy");
        if (len % 2 || len < 6)
          return invalid(who, "xy: " + at + "a polygon of " + std::to_string(len) + " numbers (an even count, at least 3 points)");
        for (int64_t i = 0; i < len; ++i)
          if (!std::isfinite(xy[lo + i]) || std::fabs(xy[lo + i]) > kMaskMaxCoord)
            return invalid(who, "xy: " + at + "a coordinate that is not finite or above 65536 in magnitude");
      } else {
        if (!counts) return invalid(who, "null counts");
        uint64_t sum = 0;
        for (int64_t i = 0; i < len; ++i) sum += counts[lo + i];
        if (sum != (uint64_t)pixels)
          return invalid(who, "counts: " + at + "the runs sum to " + std::to_string(sum) + ", the image has " +
                              std::to_string(pixels) + " pixels");
      }
    }
  }
  // everything is valid: lay the batch out
  out->images.resize(n);
  out->anns.resize(A);
  out->parts.resize(P);
  out->edge_start.push_back(0);
  for (int f = 0; f < n; ++f) {
    MaskImage& im = out->images[f];
    im.h = hw[2 * f];
    im.w = hw[2 * f + 1];
    im.ann0 = ann_offsets[f];
    im.ann1 = ann_offsets[f + 1];
    im.out_off = out->out_bytes;
    out->out_bytes += pad16((int64_t)im.h * im.w);
    const int32_t tw = (int32_t)(((int64_t)im.h * im.w + 1 + 31) / 32), cw = (im.w + 1 + 31) / 32;
    for (int a = im.ann0; a < im.ann1; ++a) {
      MaskAnn& an = out->anns[a];
      an.role = ann_role[a];
      an.part0 = part_offsets[a];
      an.part1 = part_offsets[a + 1];
      an.pad = 0;
      an.out_off = -1;
      if ((out_ann && out_ann[a]) || (ann_frames && ann_frames[f])) {
        an.out_off = out->ann_bytes;
        out->ann_bytes += pad16((int64_t)im.h * im.w);
      }
      for (int p = an.part0; p < an.part1; ++p) {
        MaskPart& pt = out->parts[p];
        pt.plane_off = out->plane_words;
        pt.tw = tw;
        pt.pad = 0;
        out->plane_words += (int64_t)tw + cw;
        const int64_t lo = data_offsets[p], len = data_offsets[p + 1] - lo;
        if (part_kind[p] == OP_MASK_RLE) {
          MaskRle r;
          r.plane_off = pt.plane_off;
          r.data_off = (int64_t)out->counts.size();
          r.n = (int32_t)len;
          r.h = im.h;
          r.tw = tw;
          r.pad = 0;
          if (len > INT32_MAX) return invalid(who, "counts: part " + std::to_string(p) + ": too many runs");
          out->counts.insert(out->counts.end(), counts + lo, counts + lo + len);
          out->rles.push_back(r);
          continue;
        }
        const int k = (int)(len / 2);
        std::vector<int32_t> X(k + 1), Y(k + 1);
        for (int j = 0; j < k; ++j) {  // (int): truncation toward zero of a float64 product and sum
          X[j] = (int32_t)((double)kMaskUp * xy[lo + 2 * j] + 0.5);
          Y[j] = (int32_t)((double)kMaskUp * xy[lo + 2 * j + 1] + 0.5);
        }
        X[k] = X[0];
        Y[k] = Y[0];
        for (int j = 0; j < k; ++j) {
          int32_t xs = X[j], ys = Y[j], xe = X[j + 1], ye = Y[j + 1];
          const int32_t dx = std::abs(xe - xs), dy = std::abs(ys - ye);
          if (dx == 0 && dy == 0) continue;  // a single point: nothing to cross
          MaskEdge e;
          e.major = dx >= dy ? 1 : 0;
          e.flip = ((dx >= dy && xs > xe) || (dx < dy && ys > ye)) ? 1 : 0;
          if (e.flip) {
            std::swap(xs, xe);
            std::swap(ys, ye);
          }
          e.s = e.major ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
          e.plane_off = pt.plane_off;
          e.xs = xs;
          e.ys = ys;
          e.len = e.major ? dx : dy;
          e.h = im.h;
          e.w = im.w;
          e.tw = tw;
          points += e.len;
          if (points > INT32_MAX) return invalid(who, "xy: more than 2^31 - 1 upsampled outline points in the batch");
          out->edges.push_back(e);
          out->edge_start.push_back((int32_t)points);
        }
      }
    }
    // column blocks: nc * h bits and the two edge words fit kFillWords
    const int nc = std::max(1, std::min(kFillMaxCols, (32 * (kFillWords - 2)) / im.h));
    for (int c0 = 0; c0 < im.w; c0 += nc) out->blocks.push_back(MaskBlock{f, c0, std::min(nc, im.w - c0), 0});
  }
  return OP_OK;
}

void mask_launch(Job& job, const MaskHost& mh, MaskDevice* md) {
  enum { IMAGES = MaskDevice::IMAGES, ANNS = MaskDevice::ANNS, PARTS = MaskDevice::PARTS, EDGES = MaskDevice::EDGES,
         ESTART = MaskDevice::ESTART, RLES = MaskDevice::RLES, COUNTS = MaskDevice::COUNTS, BLOCKS = MaskDevice::BLOCKS,
         PLANES = MaskDevice::PLANES, OALL = MaskDevice::OALL, OMISS = MaskDevice::OMISS, OANN = MaskDevice::OANN,
         NBUF = MaskDevice::NBUF };
  const void* host[NBUF] = {mh.images.data(), mh.anns.data(), mh.parts.data(), mh.edges.data(), mh.edge_start.data(),
                            mh.rles.data(), mh.counts.data(), mh.blocks.data(), nullptr, nullptr, nullptr, nullptr};
  const size_t sizes[NBUF] = {mh.images.size() * sizeof(MaskImage), mh.anns.size() * sizeof(MaskAnn),
                              mh.parts.size() * sizeof(MaskPart), mh.edges.size() * sizeof(MaskEdge),
                              mh.edge_start.size() * sizeof(int32_t), mh.rles.size() * sizeof(MaskRle),
                              mh.counts.size() * sizeof(uint32_t), mh.blocks.size() * sizeof(MaskBlock),
                              (size_t)mh.plane_words * sizeof(uint32_t), (size_t)mh.out_bytes, (size_t)mh.out_bytes,
                              (size_t)mh.ann_bytes};
  void** d = md->d;
  for (int i = 0; i < NBUF; ++i) d[i] = job.alloc(sizes[i]);
  job.begin();
  for (int i = 0; i < NBUF; ++i)
    if (host[i]) job.upload(d[i], host[i], sizes[i]);
  job.memset(d[PLANES], 0, sizes[PLANES]);
  if (!job.ok()) return;
  MaskArgs a;
  a.images = (const MaskImage*)d[IMAGES];
  a.anns = (const MaskAnn*)d[ANNS];
  a.parts = (const MaskPart*)d[PARTS];
  a.edges = (const MaskEdge*)d[EDGES];
  a.edge_start = (const int32_t*)d[ESTART];
  a.rles = (const MaskRle*)d[RLES];
  a.counts = (const uint32_t*)d[COUNTS];
  a.blocks = (const MaskBlock*)d[BLOCKS];
  a.planes = (uint32_t*)d[PLANES];
  a.out_all = (uint8_t*)d[OALL];
  a.out_miss = (uint8_t*)d[OMISS];
  a.out_ann = (uint8_t*)d[OANN];
  a.n_edges = (int32_t)mh.edges.size();
  a.total_points = mh.edge_start.back();
  if (a.total_points > 0) {
    hipLaunchKernelGGL(mask_toggles, dim3((unsigned)(((int64_t)a.total_points + 255) / 256)), dim3(256), 0,
                       job.stream(), a);
    job.check(hipGetLastError(), "mask_toggles");
  }
  if (!mh.rles.empty() && job.ok()) {
    hipLaunchKernelGGL(mask_rle, dim3((unsigned)mh.rles.size()), dim3(256), 0, job.stream(), a);
    job.check(hipGetLastError(), "mask_rle");
  }
  if (!job.ok()) return;
  hipLaunchKernelGGL(mask_fill, dim3((unsigned)mh.blocks.size()), dim3(kFillThreads), 0, job.stream(), a);
  job.check(hipGetLastError(), "mask_fill");
}

namespace {
LastMs g_mask_last;
}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_ignore_masks(int32_t device, int32_t n, const int32_t* hw, const int32_t* ann_offsets,
                               const int32_t* ann_role, const int32_t* part_offsets, const int32_t* part_kind,
                               const int64_t* data_offsets, const double* xy, const uint32_t* counts,
                               uint8_t* const* out_all, uint8_t* const* out_miss, uint8_t* const* out_ann) {
  const char* who = "op_ignore_masks";
  MaskHost mh;
  const int rc = mask_pack(who, n, hw, ann_offsets, ann_role, part_offsets, part_kind, data_offsets, xy, counts, out_ann,
                           nullptr, &mh);
  if (rc) return rc;
  const int rd = use_device(who, device);
  if (rd) return rd;
  Job job(who, nullptr);
  MaskDevice md;
  mask_launch(job, mh, &md);
  job.end();
  job.finish("kernels");
  for (int f = 0; f < n && job.ok(); ++f) {
    const MaskImage& im = mh.images[f];
    const size_t bytes = (size_t)im.h * im.w;
    if (out_all && out_all[f]) job.download(out_all[f], md.all() + im.out_off, bytes, "mask_all download");
    if (out_miss && out_miss[f]) job.download(out_miss[f], md.miss() + im.out_off, bytes, "mask_miss download");
    for (int a = im.ann0; a < im.ann1; ++a)
      if (mh.anns[a].out_off >= 0)
        job.download(out_ann[a], md.ann() + mh.anns[a].out_off, bytes, "annotation mask download");
  }
  if (job.ok()) g_mask_last.done(device, job.ms());
  return job.status();
}

extern "C" int op_ignore_masks_last_ms(int32_t device, double* ms) {
  return g_mask_last.get("op_ignore_masks_last_ms", "op_ignore_masks", device, ms);
}
