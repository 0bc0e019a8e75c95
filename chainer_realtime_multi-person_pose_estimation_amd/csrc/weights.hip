// The layer table of models/CocoPoseNet.py and the packing of its weights into the context
// (op_set_weights): Mconv1_stageN_L1/L2 and conv5_1_CPM_L1/L2 share their input -> one conv with
// Co = 256; the stage input is the 192-channel concat buffer (cat_logical).
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "host_pack.hpp"

namespace op {

struct LayerDef {
  const char* name;
  int ci, co, k;
};

// models/CocoPoseNet.py:26-129 declaration order.
static std::vector<LayerDef> make_layers() {
  std::vector<LayerDef> v;
  static const char* bb[] = {"conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2",
                             "conv3_3", "conv3_4", "conv4_1", "conv4_2", "conv4_3_CPM", "conv4_4_CPM"};
  static const int bci[] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 256};
  static const int bco[] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 256, 128};
  for (int i = 0; i < 12; ++i) v.push_back({bb[i], bci[i], bco[i], 3});
  static std::vector<std::string> names;  // storage for generated names
  names.reserve(200);
  auto add = [&](const std::string& n, int ci, int co, int k) {
    names.push_back(n);
    v.push_back({names.back().c_str(), ci, co, k});
  };
  const char* br[2] = {"L1", "L2"};
  const int out[2] = {38, 19};
  for (int b = 0; b < 2; ++b) {
    for (int i = 1; i <= 3; ++i) add("conv5_" + std::to_string(i) + "_CPM_" + br[b], 128, 128, 3);
    add(std::string("conv5_4_CPM_") + br[b], 128, 512, 1);
    add(std::string("conv5_5_CPM_") + br[b], 512, out[b], 1);
  }
  for (int s = 2; s <= 6; ++s)
    for (int b = 0; b < 2; ++b) {
      const std::string sfx = "_stage" + std::to_string(s) + "_" + br[b];
      add("Mconv1" + sfx, 185, 128, 7);
      for (int i = 2; i <= 5; ++i) add("Mconv" + std::to_string(i) + sfx, 128, 128, 7);
      add("Mconv6" + sfx, 128, 128, 1);
      add("Mconv7" + sfx, 128, out[b], 1);
    }
  return v;
}

static const std::vector<LayerDef>& layers() {
  static std::vector<LayerDef> L = make_layers();
  return L;
}

static int layer_index(const std::string& n) {
  const auto& L = layers();
  for (size_t i = 0; i < L.size(); ++i)
    if (n == L[i].name) return (int)i;
  return -1;
}

// Logical input channel of physical channel p in the stage-input buffer (-1 = zero pad).
// Logical order is F.concat((paf 38, heat 19, feature 128)) (CocoPoseNet.py:168).
static int cat_logical(int p) {
  if (p >= kCatFeat && p < kCatFeat + 128) return 57 + (p - kCatFeat);
  if (p >= kCatHeat && p < kCatHeat + 19) return 38 + (p - kCatHeat);
  if (p >= kCatPaf && p < kCatPaf + 38) return p - kCatPaf;
  return -1;
}

// Pack Chainer W (Co, Ci, k, k) into [c8][tap][cop][8] at output-channel offset co_off.
static void pack_into(std::vector<float>& dst, std::vector<float>& bias, int cop, int cin_phys, int k, const float* W,
                      const float* b, int Co, int Ci, int co_off, bool cat_input) {
  const int c8 = cin_phys / 8, taps = k * k;
  for (int co = 0; co < Co; ++co) {
    bias[co_off + co] = b[co];
    for (int p = 0; p < cin_phys; ++p) {
      const int ci = cat_input ? cat_logical(p) : (p < Ci ? p : -1);
      if (ci < 0) continue;
      for (int t = 0; t < taps; ++t) {
        const int ky = t / k, kx = t % k;
        const float v = W[(((size_t)co * Ci + ci) * k + ky) * k + kx];
        const size_t idx = ((((size_t)(p / 8) * taps + t) * cop) + (co_off + co)) * 8 + (p % 8);
        dst[idx] = v;
      }
    }
  }
  (void)c8;
}

// Pack Chainer W (Co, Ci, k, k) into the split layout at output-channel offset co_off (host_pack.hpp);
// cat_input: physical channels of the 192-channel stage input (cat_logical).
static void pack_split_into(std::vector<uint16_t>& dst, int cop, int cin16, int k, const float* W, int Co, int Ci,
                            int co_off, bool cat_input) {
  pack_split(dst, cop, cin16, k, W, Co, Ci, co_off, [&](int p) { return cat_input ? cat_logical(p) : (p < Ci ? p : -1); });
}

static int upload(PackedConv& pc, const std::vector<float>& w, const std::vector<float>& b) {
  OP_HIP_CHECK(hipMalloc(&pc.w, w.size() * sizeof(float)));
  OP_HIP_CHECK(hipMalloc(&pc.b, b.size() * sizeof(float)));
  OP_HIP_CHECK(hipMemcpy(pc.w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
  OP_HIP_CHECK(hipMemcpy(pc.b, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
  return OP_OK;
}

static int upload_split(PackedConv& pc, const std::vector<uint16_t>& ws) {
  OP_HIP_CHECK(hipMalloc(&pc.ws, ws.size() * sizeof(uint16_t)));
  OP_HIP_CHECK(hipMemcpy(pc.ws, ws.data(), ws.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  return OP_OK;
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace op

extern "C" {

int op_layer_info(int index, const char** name, int32_t* ci, int32_t* co, int32_t* ksize) {
  const auto& L = op::layers();
  if (index < 0 || index >= (int)L.size()) return OP_ERR_INVALID;
  if (name) *name = L[index].name;
  if (ci) *ci = L[index].ci;
  if (co) *co = L[index].co;
  if (ksize) *ksize = L[index].k;
  return OP_OK;
}

double op_forward_flops(int32_t h, int32_t w) {
  double f = 0.0;
  const auto& L = op::layers();
  for (size_t i = 0; i < L.size(); ++i) {
    int div = 8;
    if (i < 2) div = 1;
    else if (i < 4) div = 2;
    else if (i < 8) div = 4;
    const double hw = (double)(h / div) * (double)(w / div);
    f += 2.0 * L[i].ci * L[i].co * L[i].k * L[i].k * hw;
  }
  return f;
}

int op_set_weights(op_ctx* c, const float* const* W, const float* const* b) {
  using namespace op;
  int rc = check_ctx(c, false);
  if (rc) return rc;
  if (!W || !b) {
    set_error("null weights");
    return OP_ERR_INVALID;
  }
  for (int i = 0; i < OP_N_LAYERS; ++i)
    if (!W[i] || !b[i]) {
      set_error(std::string("missing weights for layer ") + layers()[i].name);
      return OP_ERR_INVALID;
    }
  free_weights(c);
  const auto& L = layers();
  auto single = [&](PackedConv& pc, int li, bool cat_in) -> int {
    const LayerDef& d = L[li];
    pc.ks = d.k;
    pc.cin_phys = cat_in ? kCatStride : round_up(d.ci, 8);
    pc.cop = round_up(d.co, 64);
    pc.cin_log = d.ci;
    pc.co_log = d.co;
    pc.cin16 = cat_in ? kCatStride : round_up(d.ci, 16);
    std::vector<float> w((size_t)pc.cin_phys * d.k * d.k * pc.cop, 0.0f), bias(pc.cop, 0.0f);
    pack_into(w, bias, pc.cop, pc.cin_phys, d.k, W[li], b[li], d.co, d.ci, 0, cat_in);
    std::vector<uint16_t> ws((size_t)pc.cin16 * d.k * d.k * pc.cop * 2, 0);
    pack_split_into(ws, pc.cop, pc.cin16, d.k, W[li], d.co, d.ci, 0, cat_in);
    RC(upload_split(pc, ws));
    return upload(pc, w, bias);
  };
  auto fused = [&](PackedConv& pc, int l1, int l2, bool cat_in) -> int {
    const LayerDef& d = L[l1];
    pc.ks = d.k;
    pc.cin_phys = cat_in ? kCatStride : round_up(d.ci, 8);
    pc.cop = 2 * d.co;
    pc.cin_log = d.ci;
    pc.co_log = 2 * d.co;
    pc.cin16 = cat_in ? kCatStride : round_up(d.ci, 16);
    std::vector<float> w((size_t)pc.cin_phys * d.k * d.k * pc.cop, 0.0f), bias(pc.cop, 0.0f);
    pack_into(w, bias, pc.cop, pc.cin_phys, d.k, W[l1], b[l1], d.co, d.ci, 0, cat_in);
    pack_into(w, bias, pc.cop, pc.cin_phys, d.k, W[l2], b[l2], d.co, d.ci, d.co, cat_in);
    std::vector<uint16_t> ws((size_t)pc.cin16 * d.k * d.k * pc.cop * 2, 0);
    pack_split_into(ws, pc.cop, pc.cin16, d.k, W[l1], d.co, d.ci, 0, cat_in);
    pack_split_into(ws, pc.cop, pc.cin16, d.k, W[l2], d.co, d.ci, d.co, cat_in);
    RC(upload_split(pc, ws));
    return upload(pc, w, bias);
  };
  for (int i = 0; i < 12; ++i) RC(single(c->bb[i], i, false));
  {  // conv1_1 for the VALU kernel: [tap][ci][co]
    std::vector<float> w11(9 * 3 * 64);
    for (int co = 0; co < 64; ++co)
      for (int ci = 0; ci < 3; ++ci)
        for (int t = 0; t < 9; ++t) w11[(t * 3 + ci) * 64 + co] = W[0][(co * 3 + ci) * 9 + t];
    OP_HIP_CHECK(hipMalloc(&c->w11, w11.size() * sizeof(float)));
    OP_HIP_CHECK(hipMemcpy(c->w11, w11.data(), w11.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const char* br[2] = {"L1", "L2"};
  RC(fused(c->s1_first, layer_index("conv5_1_CPM_L1"), layer_index("conv5_1_CPM_L2"), false));
  for (int bi = 0; bi < 2; ++bi) {
    for (int k = 0; k < 3; ++k)
      RC(single(c->s1_g[bi][k], layer_index("conv5_" + std::to_string(k + 2) + "_CPM_" + br[bi]), false));
    RC(single(c->s1_last[bi], layer_index(std::string("conv5_5_CPM_") + br[bi]), false));
  }
  for (int s = 0; s < 5; ++s) {
    const std::string st = "_stage" + std::to_string(s + 2) + "_";
    RC(fused(c->st_first[s], layer_index("Mconv1" + st + "L1"), layer_index("Mconv1" + st + "L2"), true));
    for (int bi = 0; bi < 2; ++bi) {
      for (int k = 0; k < 5; ++k) RC(single(c->st_g[s][bi][k], layer_index("Mconv" + std::to_string(k + 2) + st + br[bi]), false));
      RC(single(c->st_last[s][bi], layer_index("Mconv7" + st + br[bi]), false));
    }
  }
  c->have_weights = true;
  return OP_OK;
}

}  // extern "C"
