// What masks.hip shares with maskview.hip: the packed batch of op_ignore_masks and the launch of its
// three kernels, so that the annotation views read the masks where mask_fill left them in HBM.
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"
#include "oneshot.hpp"

namespace op {

struct MaskImage {
  int64_t out_off;  // into the mask_all / mask_miss buffers
  int32_t h, w, ann0, ann1;
};
struct MaskAnn {
  int64_t out_off;  // into the per-annotation buffer; < 0: not wanted
  int32_t role, part0, part1, pad;
};
struct MaskPart {
  int64_t plane_off;  // words; the column bits follow the tw toggle words
  int32_t tw, pad;
};
struct MaskEdge {
  double s;
  int64_t plane_off;
  int32_t xs, ys, len, major, flip, h, w, tw;  // len = max(dx, dy): the points 1 .. len
};
struct MaskRle {
  int64_t plane_off, data_off;
  int32_t n, h, tw, pad;
};
struct MaskBlock {
  int32_t image, c0, nc, pad;
};

struct MaskHost {
  std::vector<MaskImage> images;
  std::vector<MaskAnn> anns;
  std::vector<MaskPart> parts;
  std::vector<MaskEdge> edges;
  std::vector<int32_t> edge_start;
  std::vector<MaskRle> rles;
  std::vector<uint32_t> counts;
  std::vector<MaskBlock> blocks;
  int64_t plane_words = 0, out_bytes = 0, ann_bytes = 0;
};

// The batch on the device: the tables, the toggle planes and the row-major u8 masks (mask_all and
// mask_miss of image f at all / miss + images[f].out_off, annotation a's own mask at
// ann + anns[a].out_off where that is >= 0), in buffers of the job that launched it.
struct MaskDevice {
  enum { IMAGES, ANNS, PARTS, EDGES, ESTART, RLES, COUNTS, BLOCKS, PLANES, OALL, OMISS, OANN, NBUF };
  void* d[NBUF] = {};
  const uint8_t* all() const { return (const uint8_t*)d[OALL]; }
  const uint8_t* miss() const { return (const uint8_t*)d[OMISS]; }
  const uint8_t* ann() const { return (const uint8_t*)d[OANN]; }
};

// "entry i must start at 0 and never decrease" for count + 1 offsets (one of o64 / o32); the message
// begins with `who`.
int mask_offsets(const char* who, const char* name, const int64_t* o64, const int32_t* o32, int64_t count);

// Validates the segmentation arguments of op_ignore_masks (OP_ERR_INVALID, `who` leads the message)
// and lays the batch out; makes no HIP call.  An annotation's own mask is kept when out_ann[a] is
// set or, with ann_frames, when ann_frames[its image] is.
int mask_pack(const char* who, int32_t n, const int32_t* hw, const int32_t* ann_offsets, const int32_t* ann_role,
              const int32_t* part_offsets, const int32_t* part_kind, const int64_t* data_offsets, const double* xy,
              const uint32_t* counts, uint8_t* const* out_ann, uint8_t* const* ann_frames, MaskHost* out);

// On the current device: allocates md's buffers from the job, begins its timing, uploads mh and
// queues mask_toggles, mask_rle and mask_fill on its stream.  It does not wait; a failure is the job's.
void mask_launch(Job& job, const MaskHost& mh, MaskDevice* md);

}  // namespace op
