// The activation arena, the forward plan with its probe points, and the C ABI of the forward.
//
// The forward plan is the layer sequence of models/CocoPoseNet.py:132-262 with the two refinement
// branches fused:
//   * Mconv1_stageN_L1/L2 and conv5_1_CPM_L1/L2 share their input -> one conv with Co = 256;
//   * the later branch layers run as one 2-group launch (grid.z = branch);
//   * F.concat((paf, heat, feature)) is a single 192-channel buffer whose slices the producing
//     convs write directly (no concat copy).
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "common.hpp"
#include "ctx.hpp"

namespace op {

static size_t geom_floats(op_ctx* c, int n, int h, int w, Act* out, bool split) {
  // (pad, channel stride, scale divisor) per buffer
  struct D {
    int pad, cs, div;
  };
  const D d[B_COUNT] = {{1, 8, 1},   {1, 64, 1},  {0, 64, 1},  {1, 64, 2},  {1, 128, 2}, {0, 128, 2},
                        {1, 128, 4}, {1, 256, 4}, {1, 256, 4}, {0, 256, 4}, {1, 256, 8}, {1, 512, 8},
                        {1, 512, 8}, {1, 256, 8}, {kStagePad, kCatStride, 8}, {kStagePad, 256, 8},
                        {kStagePad, 256, 8}, {0, 1024, 8}, {0, 64, 8}, {kStagePad, 256, 8}, {kStagePad, 256, 8},
                        {kStagePad, kCatStride, 8}};
  size_t total = 0;
  for (int i = 0; i < B_COUNT; ++i) {
    Act a;
    a.pad = d[i].pad;
    a.cs = (i == B_X0 && split) ? 16 : d[i].cs;
    a.h = h / d[i].div;
    a.w = w / d[i].div;
    a.planar = (i == B_PA || i == B_PB || i == B_CATP) ? 1 : 0;  // the 7x7 inputs of stages 2-6
    const size_t fl = a.frame_floats() * (size_t)n;
    if (out) {
      out[i] = a;
      out[i].p = nullptr;
    }
    total += (fl + 63) / 64 * 64 + g_guard / 4;  // 256-B alignment (+ debug guard band)
  }
  (void)c;
  return total;
}

int ensure_geometry(op_ctx* c, int n, int h, int w) {
  if (h % 8 || w % 8 || h < 16 || w < 16 || n < 1) {
    set_error("network input must be >= 16 and a multiple of 8");
    return OP_ERR_INVALID;
  }
  if (c->gn == n && c->gh == h && c->gw == w && c->gsplit == c->split) return OP_OK;
  Act a[B_COUNT];
  const size_t need = geom_floats(c, n, h, w, a, c->split) * sizeof(float);
  op_ctx::GeomArena* ga = nullptr;
  for (auto& e : c->arenas)
    if (e.n == n && e.h == h && e.w == w && e.split == c->split) ga = &e;
  if (!ga) {
    // bounded cache: at most 6 geometries / 96 GiB of arenas, least recently used evicted first
    const size_t cap_bytes = (size_t)96 << 30;
    for (;;) {
      size_t tot = need;
      for (auto& e : c->arenas) tot += e.bytes;
      if (c->arenas.empty() || (c->arenas.size() < 6 && tot <= cap_bytes)) break;
      size_t lru = 0;
      for (size_t i = 1; i < c->arenas.size(); ++i)
        if (c->arenas[i].used < c->arenas[lru].used) lru = i;
      // every stream that may still read the arena: the compute stream and the upload ring's copy
      // stream (which touches only d_ring, but hipFree must not race any queued work)
      OP_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (c->main_stream) OP_HIP_CHECK(hipStreamSynchronize(c->main_stream));
      if (c->side_stream) OP_HIP_CHECK(hipStreamSynchronize(c->side_stream));
      if (c->copy_stream) OP_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
      guard_forget(c->arenas[lru].p, c->arenas[lru].bytes);
      OP_HIP_CHECK(hipFree(c->arenas[lru].p));
      c->arenas.erase(c->arenas.begin() + lru);
    }
    void* p = nullptr;
    OP_HIP_CHECK(hipMalloc(&p, need));
    // zero halos (and everything else) once per geometry; kernels only ever write interiors
    OP_HIP_CHECK(hipMemsetAsync(p, 0, need, c->stream));
    c->arenas.push_back(op_ctx::GeomArena{n, h, w, c->split, p, need, 0});
    ga = &c->arenas.back();
  }
  ga->used = ++c->arena_clock;
  if (c->arena) guard_forget(c->arena, c->arena_bytes);
  c->arena = ga->p;
  c->arena_bytes = ga->bytes;
  float* p = (float*)c->arena;
  for (int i = 0; i < B_COUNT; ++i) {
    a[i].p = p;
    const size_t fl = a[i].frame_floats() * (size_t)n;
    p += (fl + 63) / 64 * 64;
    guard_add(kBufName[i], p, c->stream);
    p += g_guard / 4;
    c->buf[i] = a[i];
  }
  c->gn = n;
  c->gh = h;
  c->gw = w;
  c->gsplit = c->split;
  return OP_OK;
}

// ---- forward plan ----
static ConvGroup grp(const Act& in, int cin_off, const Act& out, int cout_off, const PackedConv& pc, int cout_store) {
  ConvGroup g;
  g.in = in.p + cin_off;
  g.out = out.p + cout_off;
  g.w = pc.w;
  g.bias = pc.b;
  g.cop = pc.cop;
  g.cout_store = cout_store;
  return g;
}

static ConvShape shp(int n, const Act& in, const Act& out, int c8, int ks, bool relu, int groups) {
  ConvShape s;
  s.n = n;
  s.h = out.h;
  s.w = out.w;
  s.pin = in.pad;
  s.cs_in = in.cs;
  s.pout = out.pad;
  s.cs_out = out.cs;
  s.c8 = c8;
  s.ks = ks;
  s.relu = relu ? 1 : 0;
  s.groups = groups;
  return s;
}

static int conv_class(int ks) { return ks == 7 ? 0 : (ks == 3 ? 1 : 2); }

// algorithmic work of one conv group: 2*Ci*Co*k*k*N*H*W FLOPs; bytes = input + output + weights (fp32)
static void conv_work(const op_ctx* c, const Act& out, const PackedConv& pc, double* flops, double* bytes) {
  const double px = (double)c->gn * out.h * out.w;
  *flops += 2.0 * pc.cin_log * pc.co_log * pc.ks * pc.ks * px;
  *bytes += 4.0 * (px * pc.cin_log + px * pc.co_log + (double)pc.cin_log * pc.co_log * pc.ks * pc.ks + pc.co_log);
}

// first channel `off` (a multiple of 8) of a split tensor, in floats from its base, for its layout
static size_t chan_offset(const Act& a, int off) {
  return a.planar ? (size_t)off * (a.h + 2 * a.pad) * (a.w + 2 * a.pad) : (size_t)off;
}

static SplitConvGroup sgrp(const Act& in, int cin_off, const Act& out, int cout_off, const PackedConv& pc,
                          int cout_store) {
  SplitConvGroup g;
  g.in = in.p + chan_offset(in, cin_off);
  g.out = out.p + chan_offset(out, cout_off);
  g.w = pc.ws;
  g.bias = pc.b;
  g.cop = pc.cop;
  g.cout_store = cout_store;
  g.cin_off = cin_off;
  g.out32 = nullptr;
  g.out32_off = 0;
  return g;
}

static SplitConvShape sshp(int n, const Act& in, const Act& out, int c16, int ks, bool relu, int groups, int algo,
                           int splitk) {
  SplitConvShape s;
  s.n = n;
  s.h = out.h;
  s.w = out.w;
  s.pin = in.pad;
  s.cs_in = in.cs;
  s.pout = out.pad;
  s.cs_out = out.cs;
  s.c16 = c16;
  s.ks = ks;
  s.relu = relu ? 1 : 0;
  s.groups = groups;
  s.cs_out32 = 0;
  s.halo_mode = algo == 5 ? 4 : algo;  // 5: the default family without the register-weight kernels
  s.regw = algo == 4 ? 1 : 0;
  s.splitk = splitk;
  s.in_planar = in.planar;
  s.out_planar = out.planar;
  return s;
}

static int conv1(op_ctx* c, const Act& in, int cin_off, const Act& out, int cout_off, const PackedConv& pc, int store,
                 bool relu) {
  if (c->split) {
    SplitConvGroup g[2];
    g[0] = sgrp(in, cin_off, out, cout_off, pc, store);
    g[1] = g[0];
    double fl = 0, by = 0;
    conv_work(c, out, pc, &fl, &by);
    return profiled(c, conv_class(pc.ks), fl, by, [&] {
      return launch_conv_bf16x3(sshp(c->gn, in, out, pc.cin16 / 16, pc.ks, relu, 1, c->conv_algo, c->splitk), g, c->stream);
    });
  }
  ConvGroup g[2];
  g[0] = grp(in, cin_off, out, cout_off, pc, store);
  g[1] = g[0];
  double fl = 0, by = 0;
  conv_work(c, out, pc, &fl, &by);
  return profiled(c, conv_class(pc.ks), fl, by,
                  [&] { return launch_conv(shp(c->gn, in, out, pc.cin_phys / 8, pc.ks, relu, 1), g, c->stream); });
}

static int pool(op_ctx* c, const Act& in, const Act& out, int ch);

// conv (3x3, ReLU) followed by F.max_pooling_2d(2) (CocoPoseNet.py:137-138, 140-141, 145-146):
// one fused launch on the split path with the conv_big families (the pooled tensor is the only
// output), else the conv into `full` and the pool kernel.
static int conv_pool(op_ctx* c, const Act& in, const Act& full, const Act& pooled, const PackedConv& pc, int ch) {
  if (c->split && (c->conv_algo == 4 || c->conv_algo == 5)) {
    SplitConvGroup g[2];
    g[0] = sgrp(in, 0, pooled, 0, pc, ch);
    g[1] = g[0];
    SplitConvShape sh = sshp(c->gn, in, full, pc.cin16 / 16, pc.ks, true, 1, c->conv_algo, c->splitk);
    sh.pout = pooled.pad;
    sh.cs_out = pooled.cs;
    double fl = 0, by = 0;
    conv_work(c, full, pc, &fl, &by);
    int taken = 0;
    const int rc = profiled(c, conv_class(pc.ks), fl, by, [&] {
      return launch_conv_big_pool(sh, g, c->stream, &taken);
    });
    if (rc || taken) return rc;
  }
  const int rc = conv1(c, in, 0, full, 0, pc, ch, true);
  return rc ? rc : pool(c, full, pooled, ch);
}

static int conv2(op_ctx* c, const Act& in, int ci0, int ci1, const Act& out, int co0, int co1, const PackedConv& p0,
                 const PackedConv& p1, int st0, int st1, bool relu, const Act* out32 = nullptr, int o32a = 0,
                 int o32b = 0) {
  if (c->split) {
    SplitConvGroup g[2];
    g[0] = sgrp(in, ci0, out, co0, p0, st0);
    g[1] = sgrp(in, ci1, out, co1, p1, st1);
    SplitConvShape sh = sshp(c->gn, in, out, p0.cin16 / 16, p0.ks, relu, 2, c->conv_algo, c->splitk);
    if (out32) {
      g[0].out32 = g[1].out32 = out32->p;
      g[0].out32_off = o32a;
      g[1].out32_off = o32b;
      sh.cs_out32 = out32->cs;
    }
    double fl = 0, by = 0;
    conv_work(c, out, p0, &fl, &by);
    conv_work(c, out, p1, &fl, &by);
    return profiled(c, conv_class(p0.ks), fl, by, [&] { return launch_conv_bf16x3(sh, g, c->stream); });
  }
  ConvGroup g[2];
  g[0] = grp(in, ci0, out, co0, p0, st0);
  g[1] = grp(in, ci1, out, co1, p1, st1);
  double fl = 0, by = 0;
  conv_work(c, out, p0, &fl, &by);
  conv_work(c, out, p1, &fl, &by);
  return profiled(c, conv_class(p0.ks), fl, by,
                  [&] { return launch_conv(shp(c->gn, in, out, p0.cin_phys / 8, p0.ks, relu, 2), g, c->stream); });
}

// Fused 1x1 pair per branch (conv5_4+conv5_5, Mconv6+Mconv7): in -> a (ReLU) -> b -> out, the
// intermediate kept on chip (conv_head.hip).  Returns -1 when not taken (the caller then runs the
// two convs through `mid`).  OP_HEAD_FUSED=0 disables it (A/B).
static bool head_fused_on() {  // read per forward (not cached): the parity tests A/B it in-process
  const char* e = getenv("OP_HEAD_FUSED");
  return !(e && atoi(e) == 0);
}

static int head2(op_ctx* c, const Act& in, int ci0, int ci1, const Act& out, int co0, int co1,
                 const PackedConv* a, const PackedConv* b, int st0, int st1, const Act* out32, int o32a, int o32b) {
  if (!head_fused_on()) return -1;
  if (!c->split) {  // exact f32: conv_head_f32 (bit-identical to the two conv2 launches)
    if (out32 || a[0].ks != 1 || b[0].ks != 1 || a[0].cop % 128 || a[0].cop != a[1].cop ||
        b[0].cin_phys != a[0].cop || b[1].cin_phys != a[1].cop || b[0].cop != b[1].cop)
      return -1;
    HeadF32Shape s;
    s.n = c->gn;
    s.h = out.h;
    s.w = out.w;
    s.pin = in.pad;
    s.cs_in = in.cs;
    s.pout = out.pad;
    s.cs_out = out.cs;
    s.c8 = a[0].cin_phys / 8;
    s.co1 = a[0].cop;
    s.groups = 2;
    HeadF32Group g[2];
    const int cis[2] = {ci0, ci1}, cos[2] = {co0, co1}, sts[2] = {st0, st1};
    for (int i = 0; i < 2; ++i) {
      g[i].in = in.p + cis[i];
      g[i].w1 = a[i].w;
      g[i].b1 = a[i].b;
      g[i].cop1 = a[i].cop;
      g[i].w2 = b[i].w;
      g[i].b2 = b[i].b;
      g[i].cop2 = b[i].cop;
      g[i].out = out.p + cos[i];
      g[i].cout_store = sts[i];
    }
    double fl = 0, by = 0;
    for (int i = 0; i < 2; ++i) {
      conv_work(c, out, a[i], &fl, &by);
      conv_work(c, out, b[i], &fl, &by);
    }
    const int rc = profiled(c, 2, fl, by, [&] { return launch_conv_head_f32(s, g, c->stream); });
    return rc ? rc : 0;
  }
  HeadShape s;
  s.n = c->gn;
  s.h = out.h;
  s.w = out.w;
  s.pin = in.pad;
  s.cs_in = in.cs;
  s.pout = out.pad;
  s.cs_out = out.cs;
  s.ci = a[0].cin16;
  s.co1 = a[0].cop;
  s.groups = 2;
  s.cs_out32 = out32 ? out32->cs : 0;
  s.in_planar = in.planar;
  s.out_planar = out.planar;
  HeadGroup g[2];
  const int cis[2] = {ci0, ci1}, cos[2] = {co0, co1}, sts[2] = {st0, st1}, o32[2] = {o32a, o32b};
  for (int i = 0; i < 2; ++i) {
    g[i].in = in.p + chan_offset(in, cis[i]);
    g[i].w1 = a[i].ws;
    g[i].b1 = a[i].b;
    g[i].cop1 = a[i].cop;
    g[i].w2 = b[i].ws;
    g[i].b2 = b[i].b;
    g[i].cop2 = b[i].cop;
    g[i].out = out.p + chan_offset(out, cos[i]);
    g[i].cout_store = sts[i];
    g[i].out32 = out32 ? out32->p : nullptr;
    g[i].out32_off = o32[i];
  }
  double fl = 0, by = 0;
  for (int i = 0; i < 2; ++i) {
    conv_work(c, out, a[i], &fl, &by);
    conv_work(c, out, b[i], &fl, &by);
  }
  int taken = 0;
  const int rc = profiled(c, 2, fl, by, [&] { return launch_conv_head(s, g, c->stream, &taken); });
  return rc ? rc : (taken ? 0 : -1);
}

static int pool(op_ctx* c, const Act& in, const Act& out, int ch) {
  return profiled(c, kProfOther, 0.0, 0.0, [&] {
    if (c->split) return launch_maxpool2_split(in.p, in.pad, out.p, out.pad, c->gn, in.h, in.w, ch, c->stream);
    return launch_maxpool2(in.p, in.pad, out.p, out.pad, c->gn, in.h, in.w, ch, c->stream);
  });
}

// Whether this forward runs stages 2-6 on the chunk-planar buffers (see run_forward).
static bool stages_planar(const op_ctx* c) {
  const int sh8 = c->buf[B_BRA].h, sw8 = c->buf[B_BRA].w;
  return c->split && (c->conv_algo == 4 || c->conv_algo == 5) && c->stage_planar && head_fused_on() &&
         conv_m16_takes(c->gn, sh8, sw8, 1, 256) && conv_m16_takes(c->gn, sh8, sw8, 2, 128);
}

// ---- probe points (op_forward_probe): the launch boundaries of run_forward in execution order ----
// (name, channels returned, size divisor); map points return paf 38 | heat 19 | feature 128, the
// reference's F.concat order (CocoPoseNet.py:168)
struct ProbeInfo {
  const char* name;
  int channels, div;
};
constexpr int kProbePoints = 46;
static ProbeInfo probe_info(int point) {
  static const ProbeInfo head[16] = {
      {"input", 3, 1},          {"conv1_2+pool", 64, 2},  {"conv2_1", 128, 2},      {"conv2_2+pool", 128, 4},
      {"conv3_1", 256, 4},      {"conv3_2", 256, 4},      {"conv3_3", 256, 4},      {"conv3_4+pool", 256, 8},
      {"conv4_1", 512, 8},      {"conv4_2", 512, 8},      {"conv4_3_CPM", 256, 8},  {"conv4_4_CPM", 128, 8},
      {"conv5_1", 256, 8},      {"conv5_2", 256, 8},      {"conv5_3", 256, 8},      {"stage1", 185, 8}};
  if (point < 16) return head[point];
  static const char* const names[5][6] = {
      {"Mconv1_stage2", "Mconv2_stage2", "Mconv3_stage2", "Mconv4_stage2", "Mconv5_stage2", "stage2"},
      {"Mconv1_stage3", "Mconv2_stage3", "Mconv3_stage3", "Mconv4_stage3", "Mconv5_stage3", "stage3"},
      {"Mconv1_stage4", "Mconv2_stage4", "Mconv3_stage4", "Mconv4_stage4", "Mconv5_stage4", "stage4"},
      {"Mconv1_stage5", "Mconv2_stage5", "Mconv3_stage5", "Mconv4_stage5", "Mconv5_stage5", "stage5"},
      {"Mconv1_stage6", "Mconv2_stage6", "Mconv3_stage6", "Mconv4_stage6", "Mconv5_stage6", "stage6"}};
  const int st = (point - 16) / 6, i = (point - 16) % 6;
  return ProbeInfo{names[st][i], i == 5 ? 185 : 256, 8};
}

// Extract what probe point `point` wrote (frames [f0, f0 + nf)) as dense f32 NCHW into d_out.
static int probe_extract(op_ctx* c, int point, int f0, int nf, float* d_out) {
  const Act* B = c->buf;
  const bool planar = stages_planar(c);
  auto view = [&](const Act& a) { return ActView{c->split ? (a.planar ? 2 : 1) : 0, a.pad, a.cs, a.h, a.w}; };
  auto take = [&](const Act& a, int c0, int nc, int dst_c0, int dst_ch) {
    return launch_extract_act(a.p, view(a), c->gn, f0, nf, c0, nc, d_out, dst_c0, dst_ch, c->stream);
  };
  const int i = point < 16 ? -1 : (point - 16) % 6;
  if (point == 15 || i == 5) {  // the buffer the next stage's Mconv1 reads
    const Act& m = planar ? B[B_CATP] : B[B_CAT];
    RC(take(m, kCatPaf, 38, 0, 185));
    RC(take(m, kCatHeat, 19, 38, 185));
    return take(m, kCatFeat, 128, 57, 185);
  }
  if (point >= 16) {  // Mconv1, 3, 5 write SA, Mconv2, 4 SB
    const Act& a = (i % 2 == 0) ? (planar ? B[B_PA] : B[B_BRA]) : (planar ? B[B_PB] : B[B_BRB]);
    return take(a, 0, 256, 0, 256);
  }
  static const int buf_of[15] = {B_X0, B_P1, B_C21, B_P2, B_C3A, B_C3B, B_C3A, B_P3, B_C41, B_C42, B_C43, B_CAT,
                                 B_BRA, B_BRB, B_BRA};
  const int nc = probe_info(point).channels;
  return take(B[buf_of[point]], point == 11 ? kCatFeat : 0, nc, 0, nc);
}

// frames != nullptr (split path): conv1_1 reads the uint8 frames directly (fused input kernel).
// stages != nullptr: every stage's (paf, heat) is also extracted to stages = paf [6][n][38][lh][lw]
// followed by heat [6][n][19][lh][lw] (op_forward_stages; the reference's pafs / heatmaps lists).
// stop_point >= 0 (op_forward_probe only): return right after probe point stop_point (kProbe); the
// default never matches the point counter, so every other caller launches the whole forward.
int run_forward(op_ctx* c, const uint8_t* frames, int64_t frame_bytes, int64_t row_stride, int sh, int sw,
                float* stages, int stop_point) {
  c->post_rec.kind = 0;  // the maps a recorded post-process read are overwritten from here on
  Act* B = c->buf;
  int point = 0;  // probe points passed so far (point 0 is the network input, already in B_X0)
  if (stop_point == 0) return OP_OK;
// the launches of probe point `point + 1` are enqueued: stop here when it is the probed one
#define PROBE_POINT()                 \
  do {                                \
    if (++point == stop_point) {      \
      c->prof_join = false;           \
      return OP_OK;                   \
    }                                 \
  } while (0)
  const size_t stage_px = (size_t)c->gn * (c->gh / 8) * (c->gw / 8);
  auto dump_stage = [&](int s) -> int {
    if (!stages) return OP_OK;
    float* paf = stages + (size_t)s * 38 * stage_px;
    float* heat = stages + (size_t)6 * 38 * stage_px + (size_t)s * 19 * stage_px;
    if (c->split) return launch_extract_maps32(B[B_MAP32].p, 64, 40, c->gn, c->gh / 8, c->gw / 8, paf, heat, c->stream);
    return launch_extract_maps(B[B_CAT].p, c->gn, c->gh / 8, c->gw / 8, paf, heat, c->stream);
  };
  static const bool c11_mfma = getenv("OP_CONV11_MFMA") != nullptr;  // debugging aid: the MFMA conv1_1
  // conv1_1 + conv1_2 + pool in one launch (conv1_pair.hip); OP_CONV1_FUSED=0: the two-kernel path
  static const bool c1_fused = !(getenv("OP_CONV1_FUSED") && atoi(getenv("OP_CONV1_FUSED")) == 0);
  bool conv1_done = false;
  if (c->split && c1_fused && !c11_mfma && (c->conv_algo == 4 || c->conv_algo == 5)) {
    const Act& o = B[B_C11];
    double fl = 0, by = 0;
    conv_work(c, o, c->bb[0], &fl, &by);
    conv_work(c, o, c->bb[1], &fl, &by);
    RC(profiled(c, conv_class(3), fl, by, [&] {
      return launch_conv1_pair(frames, frame_bytes, row_stride, sh, sw, B[B_X0].p, c->gn, o.h, o.w, c->w11,
                               c->bb[0].b, c->bb[1].ws, c->bb[1].b, B[B_P1].p, B[B_P1].pad, c->stream);
    }));
    conv1_done = true;
  } else if (c->split && !(c11_mfma && !frames)) {
    const Act& o = B[B_C11];
    double fl = 0, by = 0;
    conv_work(c, o, c->bb[0], &fl, &by);
    RC(profiled(c, conv_class(3), fl, by, [&] {
      return launch_conv11_split(frames, frame_bytes, row_stride, sh, sw, B[B_X0].p, c->gn, o.h, o.w, c->w11,
                                 c->bb[0].b, o.p, c->stream);
    }));
  } else {
    RC(conv1(c, B[B_X0], 0, B[B_C11], 0, c->bb[0], 64, true));
  }
  if (!conv1_done) RC(conv_pool(c, B[B_C11], B[B_C12], B[B_P1], c->bb[1], 64));
  PROBE_POINT();  // 1
  RC(conv1(c, B[B_P1], 0, B[B_C21], 0, c->bb[2], 128, true));
  PROBE_POINT();
  RC(conv_pool(c, B[B_C21], B[B_C22], B[B_P2], c->bb[3], 128));
  PROBE_POINT();
  RC(conv1(c, B[B_P2], 0, B[B_C3A], 0, c->bb[4], 256, true));
  PROBE_POINT();
  RC(conv1(c, B[B_C3A], 0, B[B_C3B], 0, c->bb[5], 256, true));
  PROBE_POINT();
  RC(conv1(c, B[B_C3B], 0, B[B_C3A], 0, c->bb[6], 256, true));
  PROBE_POINT();
  RC(conv_pool(c, B[B_C3A], B[B_C34], B[B_P3], c->bb[7], 256));
  PROBE_POINT();  // 7
  RC(conv1(c, B[B_P3], 0, B[B_C41], 0, c->bb[8], 512, true));
  PROBE_POINT();
  RC(conv1(c, B[B_C41], 0, B[B_C42], 0, c->bb[9], 512, true));
  PROBE_POINT();
  RC(conv1(c, B[B_C42], 0, B[B_C43], 0, c->bb[10], 256, true));
  PROBE_POINT();
  RC(conv1(c, B[B_C43], 0, B[B_CAT], kCatFeat, c->bb[11], 128, true));
  PROBE_POINT();  // 11
  // Stages 2-6 run their 7x7 layers on chunk-planar tensors when conv_m16_bf16x3 takes every 7x7
  // launch of this geometry and the fused heads write the stage maps (op_set_stage_layout(ctx, 0)
  // or OP_STAGE_PLANAR=0: the [pixel][channels] buffers): Mconv1..Mconv5 outputs in PA / PB, and the Mconv1 input
  // (the 185-channel concat) in CATP -- the feature slice copied over from CAT once per forward
  // (stage 1's conv5_1 reads it from CAT), every stage's (paf, heat) written there by its head.
  const int sh8 = B[B_BRA].h, sw8 = B[B_BRA].w;
  const bool planar = stages_planar(c);
  if (planar)
    RC(profiled(c, kProfOther, 0.0, 0.0, [&] {
      return launch_split_to_planar(B[B_CAT].p, B[B_CATP].p, c->gn, sh8, sw8, B[B_CAT].pad, B[B_CAT].cs, 128 / 16,
                                    c->stream);
    }));
  const Act& catm = planar ? B[B_CATP] : B[B_CAT];  // stage maps + Mconv1 input
  // stage 1 (CocoPoseNet.py:153-165)
  const Act& cat = B[B_CAT];
  Act s1 = B[B_S1];
  RC(conv1(c, cat, kCatFeat, B[B_BRA], 0, c->s1_first, 256, true));
  PROBE_POINT();
  RC(conv2(c, B[B_BRA], 0, 128, B[B_BRB], 0, 128, c->s1_g[0][0], c->s1_g[1][0], 128, 128, true));
  PROBE_POINT();
  RC(conv2(c, B[B_BRB], 0, 128, B[B_BRA], 0, 128, c->s1_g[0][1], c->s1_g[1][1], 128, 128, true));
  PROBE_POINT();  // 14
  {
    const Act* m32 = (c->split && stages) ? &B[B_MAP32] : nullptr;
    const PackedConv a[2] = {c->s1_g[0][2], c->s1_g[1][2]}, b[2] = {c->s1_last[0], c->s1_last[1]};
    const int h = head2(c, B[B_BRA], 0, 128, catm, kCatPaf, kCatHeat, a, b, 40, 20, m32, 0, 40);
    if (h > 0) return h;
    if (h < 0) {
      RC(conv2(c, B[B_BRA], 0, 128, s1, 0, 512, c->s1_g[0][2], c->s1_g[1][2], 512, 512, true));
      RC(conv2(c, s1, 0, 512, catm, kCatPaf, kCatHeat, c->s1_last[0], c->s1_last[1], 40, 20, false, m32, 0, 40));
    }
    RC(dump_stage(0));
    PROBE_POINT();  // 15
  }
  // stages 2-6 (CocoPoseNet.py:167-260), on the chunk-planar buffers when `planar` (above)
  Act s6 = B[B_S1];
  s6.cs = 256;  // Mconv6 output reuses the stage-1 1x1 buffer (no halo) with a 256-channel stride
  const Act& SA = planar ? B[B_PA] : B[B_BRA];
  const Act& SB = planar ? B[B_PB] : B[B_BRB];
  for (int st = 0; st < 5; ++st) {
    RC(conv1(c, catm, 0, SA, 0, c->st_first[st], 256, true));
    PROBE_POINT();  // 16 + 6 st
    const Act* src = &SA;
    const Act* dst = &SB;
    c->prof_join = true;  // Mconv2..Mconv5 follow Mconv1 back to back on the stream
    for (int i = 0; i < 4; ++i) {
      const int r = conv2(c, *src, 0, 128, *dst, 0, 128, c->st_g[st][0][i], c->st_g[st][1][i], 128, 128, true);
      if (r) {
        c->prof_join = false;
        return r;
      }
      std::swap(src, dst);
      PROBE_POINT();  // restores prof_join
    }
    c->prof_join = false;
    // the last stage also leaves a dense f32 copy (paf at 0, heat at 40) for the post-process
    const Act* m32 = (c->split && (st == 4 || stages)) ? &B[B_MAP32] : nullptr;
    const PackedConv a[2] = {c->st_g[st][0][4], c->st_g[st][1][4]}, b[2] = {c->st_last[st][0], c->st_last[st][1]};
    const int h = head2(c, *src, 0, 128, catm, kCatPaf, kCatHeat, a, b, 40, 20, m32, 0, 40);
    if (h > 0) return h;
    if (h < 0) {
      RC(conv2(c, *src, 0, 128, s6, 0, 128, c->st_g[st][0][4], c->st_g[st][1][4], 128, 128, true));
      RC(conv2(c, s6, 0, 128, catm, kCatPaf, kCatHeat, c->st_last[st][0], c->st_last[st][1], 40, 20, false, m32, 0,
               40));
    }
    RC(dump_stage(st + 1));
    PROBE_POINT();  // 21 + 6 st
  }
#undef PROBE_POINT
  return OP_OK;
}

}  // namespace op

extern "C" {

int op_preprocess(op_ctx* c, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride, int32_t out_w,
                  int32_t out_h, float* x_out) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!bgr || !x_out || h < 1 || w < 1 || out_w < 1 || out_h < 1 || row_stride < (int64_t)w * 3) {
    set_error("op_preprocess: bad arguments");
    return OP_ERR_INVALID;
  }
  const size_t in_bytes = (size_t)h * w * 3, out_bytes = (size_t)3 * out_h * out_w * 4;
  RC(ensure_scratch(c, in_bytes + 256 + out_bytes));
  uint8_t* din = (uint8_t*)c->d_scratch;
  float* dout = (float*)((char*)c->d_scratch + (in_bytes + 255) / 256 * 256);
  OP_HIP_CHECK(hipMemcpy2DAsync(din, (size_t)w * 3, bgr, (size_t)row_stride, (size_t)w * 3, h, hipMemcpyHostToDevice,
                                c->stream));
  RC(launch_preprocess_planar(din, (int64_t)w * 3, h, w, out_h, out_w, dout, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(x_out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

int op_forward_stages(op_ctx* c, const float* x, int32_t n, int32_t h, int32_t w, float* pafs, float* heatmaps) {
  using namespace op;
  RC(check_ctx(c, true));
  if (!x || !pafs || !heatmaps) {
    set_error("op_forward_stages: null pointer");
    return OP_ERR_INVALID;
  }
  RC(ensure_geometry(c, n, h, w));
  const size_t xin = (size_t)n * 3 * h * w * 4;
  const size_t px = (size_t)n * (h / 8) * (w / 8);
  const size_t outb = 6 * 57 * px * 4;
  RC(ensure_scratch(c, xin + 256 + outb));
  float* dx = c->d_scratch;
  float* dst = (float*)((char*)c->d_scratch + (xin + 255) / 256 * 256);
  OP_HIP_CHECK(hipMemcpyAsync(dx, x, xin, hipMemcpyHostToDevice, c->stream));
  if (c->split)
    RC(launch_nchw_to_split16(dx, c->buf[B_X0].p, n, h, w, c->stream));
  else
    RC(launch_nchw_to_nhwc8(dx, c->buf[B_X0].p, n, h, w, c->stream));
  RC(run_forward(c, nullptr, 0, 0, 0, 0, dst));
  OP_HIP_CHECK(hipMemcpyAsync(pafs, dst, 6 * 38 * px * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(heatmaps, dst + 6 * 38 * px, 6 * 19 * px * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

int op_forward(op_ctx* c, const float* x, int32_t n, int32_t h, int32_t w, float* pafs, float* heatmaps) {
  using namespace op;
  RC(check_ctx(c, true));
  if (!x || !pafs || !heatmaps) {
    set_error("op_forward: null pointer");
    return OP_ERR_INVALID;
  }
  RC(ensure_geometry(c, n, h, w));
  const size_t xin = (size_t)n * 3 * h * w * 4;
  const int lh = h / 8, lw = w / 8;
  const size_t outb = (size_t)n * 57 * lh * lw * 4;
  RC(ensure_scratch(c, xin + 256 + outb));
  float* dx = c->d_scratch;
  float* dmaps = (float*)((char*)c->d_scratch + (xin + 255) / 256 * 256);
  OP_HIP_CHECK(hipMemcpyAsync(dx, x, xin, hipMemcpyHostToDevice, c->stream));
  if (c->split)
    RC(launch_nchw_to_split16(dx, c->buf[B_X0].p, n, h, w, c->stream));
  else
    RC(launch_nchw_to_nhwc8(dx, c->buf[B_X0].p, n, h, w, c->stream));
  RC(run_forward(c));
  float* dpaf = dmaps;
  float* dheat = dmaps + (size_t)n * 38 * lh * lw;
  if (c->split)
    RC(launch_extract_maps32(c->buf[B_MAP32].p, 64, 40, n, lh, lw, dpaf, dheat, c->stream));
  else
    RC(launch_extract_maps(c->buf[B_CAT].p, n, lh, lw, dpaf, dheat, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(pafs, dpaf, (size_t)n * 38 * lh * lw * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(heatmaps, dheat, (size_t)n * 19 * lh * lw * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

int op_forward_probe_info(int32_t point, const char** name, int32_t* channels, int32_t* divisor) {
  if (point < 0 || point >= op::kProbePoints || !name || !channels || !divisor) return OP_ERR_INVALID;
  const op::ProbeInfo p = op::probe_info(point);
  *name = p.name;
  *channels = p.channels;
  *divisor = p.div;
  return OP_OK;
}

int op_forward_probe(op_ctx* c, const float* x, int32_t n, int32_t h, int32_t w, int32_t point, int32_t frame0,
                     int32_t nframes, float* out, int64_t out_floats) {
  using namespace op;
  RC(check_ctx(c, true));
  if (!x || !out) {
    set_error("op_forward_probe: null pointer");
    return OP_ERR_INVALID;
  }
  if (point < 0 || point >= kProbePoints) {
    set_error("op_forward_probe: point must be 0 .. 45");
    return OP_ERR_INVALID;
  }
  if (h % 8 || w % 8 || h < 16 || w < 16 || n < 1) {
    set_error("network input must be >= 16 and a multiple of 8");
    return OP_ERR_INVALID;
  }
  if (frame0 < 0 || nframes < 1 || frame0 > n - nframes) {
    set_error("op_forward_probe: frames [frame0, frame0 + nframes) must lie in [0, n)");
    return OP_ERR_INVALID;
  }
  const ProbeInfo pi = probe_info(point);
  const int64_t want = (int64_t)nframes * pi.channels * (h / pi.div) * (w / pi.div);
  if (out_floats != want) {
    set_error("op_forward_probe: out_floats must be nframes * channels * (h / divisor) * (w / divisor) = " +
              std::to_string(want));
    return OP_ERR_INVALID;
  }
  RC(ensure_geometry(c, n, h, w));
  const size_t xin = (size_t)n * 3 * h * w * 4;
  RC(ensure_scratch(c, xin + 256 + (size_t)want * 4));
  float* dx = c->d_scratch;
  float* dout = (float*)((char*)c->d_scratch + (xin + 255) / 256 * 256);
  OP_HIP_CHECK(hipMemcpyAsync(dx, x, xin, hipMemcpyHostToDevice, c->stream));
  if (c->split)
    RC(launch_nchw_to_split16(dx, c->buf[B_X0].p, n, h, w, c->stream));
  else
    RC(launch_nchw_to_nhwc8(dx, c->buf[B_X0].p, n, h, w, c->stream));
  RC(run_forward(c, nullptr, 0, 0, 0, 0, nullptr, point));
  RC(probe_extract(c, point, frame0, nframes, dout));
  OP_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)want * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

int op_resize_images(op_ctx* c, const float* x, int32_t ch, int32_t h, int32_t w, int32_t oh, int32_t ow, float* y) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!x || !y || ch < 1 || h < 2 || w < 2 || oh < 1 || ow < 1) {
    set_error("op_resize_images: bad arguments");
    return OP_ERR_INVALID;
  }
  const size_t inb = (size_t)ch * h * w * 4, outb = (size_t)ch * oh * ow * 4;
  RC(ensure_scratch(c, inb + 256 + outb));
  float* din = c->d_scratch;
  float* dout = (float*)((char*)c->d_scratch + (inb + 255) / 256 * 256);
  OP_HIP_CHECK(hipMemcpyAsync(din, x, inb, hipMemcpyHostToDevice, c->stream));
  RC(launch_resize_images(din, ch, h, w, oh, ow, dout, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(y, dout, outb, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

}  // extern "C"
