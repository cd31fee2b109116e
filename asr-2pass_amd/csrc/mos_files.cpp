// The DNSMOS speech-quality networks read from their own files (utils/DNSMOS/sig_bak_ovr.onnx, utils/pDNSMOS/sig_bak_ovr.onnx,
// utils/DNSMOS/model_v8.onnx; what ComputeScore.__init__ of utils/dnsmos_local.py:25-27 opens through onnxruntime) into the weight
// container pfhip_mos_create_from_memory takes.  Host code only (no HIP): the protobuf walk is model_files.cpp's.
//
// The graph is walked node by node.  Primary net: the front end must be exactly Slice, Slice, Reshape, Reshape, Concat, Conv
// (stft-real), Conv (stft-imag), Mul, Mul, Add, Sqrt, Pow, Max, Log, Div in that order (Transposes and the Unsqueeze between them move
// data only), its two 1x1 Conv kernels are told apart by their tensor NAMES (time2freq/stft-real|imag/kernel:0), and Pow / Max / Div
// each carry one scalar initialiser.  Then, for both nets: Conv (kernel 3x3, pads 1, strides 1, dilations 1, group 1, with bias) + Relu
// groups, a MaxPool (kernel 2x2, strides 2, no pads, floor, not SAME) only directly behind such a Relu, ReduceMax, and three MatMul +
// Add (+ Relu) whose weights and biases are initialisers.  Anything else is refused, naming the first node that does not fit.
//
// Container ("kind": "dnsmos"; convert.py convert_dnsmos writes the same bytes): tensors in the order <net>.stft_real [161, 320],
// <net>.stft_imag, <net>.consts [3] = (floor, power, denom) (primary only), <net>.conv<i>.w [Cout, Cin, 3, 3], .b [Cout],
// <net>.dense<i>.w [in, out], .b [out], net = primary then p808; 256-byte aligned.  config: has_p808, <net>_convs = (Cout, Cin, pool)
// triples flattened, <net>_dense = (in, out) pairs flattened.
#include <cstring>
#include <fstream>

#include "model_files.h"

namespace pfhip_files {
namespace {

[[noreturn]] void refuse(const Node& nd, const std::string& why) {
  throw FormatError("not a DNSMOS graph: node " + (nd.name.empty() ? (nd.outputs.empty() ? std::string("?") : nd.outputs[0]) : nd.name) +
                    " (" + nd.op_type + "): " + why);
}

struct Tensor {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> v;
};
struct Net {
  std::vector<Tensor> front;                      // stft_real, stft_imag, consts
  std::vector<Tensor> convs, dense;               // w, b alternating
  std::vector<int> conv_cfg, dense_cfg;
};

const Initializer* init_of(const OnnxModel& m, const std::string& name) {
  auto it = m.initializers.find(name);
  return it == m.initializers.end() || it->second.external ? nullptr : &it->second;
}
bool floats_of(const Initializer& t, std::vector<float>& out) {
  if (t.dtype != 1) return false;
  const size_t n = t.count();
  out.resize(n);
  if (t.raw) {
    if (t.raw_bytes != n * 4) return false;
    if (n) std::memcpy(out.data(), t.raw, n * 4);
  } else {
    if (t.f32.size() != n) return false;
    out = t.f32;
  }
  return true;
}
std::vector<int64_t> ints_attr(const Node& nd, const char* name) {
  auto it = nd.ints_attrs.find(name);
  return it == nd.ints_attrs.end() ? std::vector<int64_t>() : it->second;
}
int64_t int_attr(const Node& nd, const char* name, int64_t dflt) {
  auto it = nd.int_attrs.find(name);
  return it == nd.int_attrs.end() ? dflt : it->second;
}
bool auto_pad_plain(const Node& nd) {
  auto it = nd.str_attrs.find("auto_pad");
  return it == nd.str_attrs.end() || it->second == "NOTSET" || it->second == "VALID";
}

void walk(const OnnxModel& m, bool primary, Net& net) {
  static const char* const kFront[] = {"Slice", "Slice", "Reshape", "Reshape", "Concat", "Conv", "Conv", "Mul", "Mul", "Add", "Sqrt", "Pow",
                                       "Max", "Log", "Div"};
  const size_t n_front = primary ? sizeof(kFront) / sizeof(kFront[0]) : 0;
  size_t at = 0;                                  // front-end nodes seen
  Tensor consts{"consts", {3}, {0.f, 0.f, 0.f}};
  Tensor wr, wi;
  std::string last_conv_out, last_relu_out, last_relu_src, dense_out;
  bool pooled = false, have_max = false;
  int stage = 0;                                  // 0 convolutions, 1 after ReduceMax
  for (const Node& nd : m.nodes) {
    const std::string& op = nd.op_type;
    if (at < n_front) {                           // ---- the primary net's front end
      if (op == "Transpose" || op == "Unsqueeze") continue;
      if (op != kFront[at]) refuse(nd, std::string("the front end needs a ") + kFront[at] + " here");
      if (op == "Conv") {
        const Initializer* w = nd.inputs.size() == 2 ? init_of(m, nd.inputs[1]) : nullptr;
        if (!w) refuse(nd, "the STFT kernel is not an initialiser of the file");
        const bool real = nd.inputs[1].find("stft-real") != std::string::npos, imag = nd.inputs[1].find("stft-imag") != std::string::npos;
        Tensor& dst = real ? wr : wi;
        if (real == imag || !dst.v.empty()) refuse(nd, "its kernel " + nd.inputs[1] + " is not named as the real or the imaginary STFT kernel");
        if (w->dims != std::vector<int64_t>{161, 320, 1} || !floats_of(*w, dst.v) || ints_attr(nd, "kernel_shape") != std::vector<int64_t>{1} ||
            ints_attr(nd, "strides") != std::vector<int64_t>{1} || int_attr(nd, "group", 1) != 1 || !auto_pad_plain(nd))
          refuse(nd, "not a [161, 320, 1] float kernel applied as a 1x1 convolution");
      } else if (op == "Pow" || op == "Max" || op == "Div") {
        const Initializer* c = nullptr;
        int n_const = 0;
        for (const std::string& in : nd.inputs)
          if (const Initializer* t = init_of(m, in)) { c = t; ++n_const; }
        std::vector<float> v;
        if (n_const != 1 || c->count() != 1 || !floats_of(*c, v)) refuse(nd, "its constant is not one scalar float initialiser");
        consts.v[op == "Max" ? 0 : op == "Pow" ? 1 : 2] = v[0];
      }
      ++at;
      continue;
    }
    if (op == "Transpose" || op == "Unsqueeze") continue;
    if (op == "Conv" && stage == 0) {
      const Initializer* w = nd.inputs.size() == 3 ? init_of(m, nd.inputs[1]) : nullptr;
      const Initializer* b = nd.inputs.size() == 3 ? init_of(m, nd.inputs[2]) : nullptr;
      if (!w) refuse(nd, "its kernel is not an initialiser of the file");
      if (!b) refuse(nd, "its bias is not an initialiser of the file");
      Tensor tw, tb;
      const std::vector<int64_t> one2{1, 1};
      const std::vector<int64_t> dil = ints_attr(nd, "dilations");
      if (w->dims.size() != 4 || w->dims[2] != 3 || w->dims[3] != 3 || w->dims[0] < 1 || w->dims[0] > 4096 || w->dims[1] < 1 || w->dims[1] > 4096 ||
          b->dims != std::vector<int64_t>{w->dims[0]} || !floats_of(*w, tw.v) || !floats_of(*b, tb.v) ||
          ints_attr(nd, "pads") != std::vector<int64_t>{1, 1, 1, 1} || ints_attr(nd, "strides") != one2 || (!dil.empty() && dil != one2) ||
          int_attr(nd, "group", 1) != 1 || !auto_pad_plain(nd))
        refuse(nd, "not a 3x3 / pads 1 / strides 1 float convolution with a bias");
      const int cin = (int)w->dims[1], cout = (int)w->dims[0];
      if (net.conv_cfg.empty() ? cin != 1 : cin != net.conv_cfg[net.conv_cfg.size() - 3])
        refuse(nd, "its input channels do not follow from the layer before");
      tw.shape = w->dims;
      tb.shape = b->dims;
      net.convs.push_back(std::move(tw));
      net.convs.push_back(std::move(tb));
      net.conv_cfg.insert(net.conv_cfg.end(), {cout, cin, 0});
      last_conv_out = nd.outputs.empty() ? "" : nd.outputs[0];
      pooled = false;
    } else if (op == "Relu") {
      if (nd.inputs.size() != 1 || nd.outputs.empty()) refuse(nd, "malformed");
      if (stage == 0 ? nd.inputs[0] != last_conv_out : (nd.inputs[0] != dense_out || net.dense.size() % 2 || net.dense.empty())) refuse(nd, "a Relu that does not follow a convolution or a dense layer");
      last_relu_out = nd.outputs[0];
      last_relu_src = nd.inputs[0];
      if (stage == 1) dense_out = nd.outputs[0];
    } else if (op == "MaxPool" && stage == 0) {
      const std::vector<int64_t> two2{2, 2};
      bool pads0 = true;
      for (int64_t p : ints_attr(nd, "pads")) pads0 = pads0 && p == 0;
      if (nd.inputs.size() != 1 || nd.inputs[0] != last_relu_out || last_relu_src != last_conv_out || pooled || net.conv_cfg.empty() ||
          ints_attr(nd, "kernel_shape") != two2 || ints_attr(nd, "strides") != two2 || !pads0 || int_attr(nd, "ceil_mode", 0) != 0 ||
          !auto_pad_plain(nd))
        refuse(nd, "not a 2x2 / strides 2 floor pool directly behind a convolution's Relu");
      net.conv_cfg.back() = 1;
      pooled = true;
      last_relu_out = nd.outputs.empty() ? "" : nd.outputs[0];      // nothing but the next Conv may follow
    } else if (op == "ReduceMax" && stage == 0 && !net.conv_cfg.empty()) {
      if (ints_attr(nd, "axes") != std::vector<int64_t>{1, 2} || int_attr(nd, "keepdims", 1) != 0) refuse(nd, "not a maximum over axes 1 and 2");
      stage = 1;
      have_max = true;
      dense_out = nd.outputs.empty() ? "" : nd.outputs[0];
    } else if (op == "MatMul" && stage == 1) {
      const Initializer* w = nd.inputs.size() == 2 ? init_of(m, nd.inputs[1]) : nullptr;
      Tensor tw;
      if (!w || nd.inputs[0] != dense_out || w->dims.size() != 2 || w->dims[0] < 1 || w->dims[0] > 256 || w->dims[1] < 1 || w->dims[1] > 256 ||
          !floats_of(*w, tw.v))
        refuse(nd, "not a dense layer (at most 256 wide) on the value before it, with its float weight in the file");
      const int in = (int)w->dims[0], out = (int)w->dims[1];
      if (net.dense_cfg.empty() ? in != net.conv_cfg[net.conv_cfg.size() - 3] : in != net.dense_cfg.back())
        refuse(nd, "its input width does not follow from the layer before");
      if (net.dense.size() % 2) refuse(nd, "the dense layer before it has no bias");
      tw.shape = w->dims;
      net.dense.push_back(std::move(tw));
      net.dense_cfg.insert(net.dense_cfg.end(), {in, out});
      dense_out = nd.outputs.empty() ? "" : nd.outputs[0];
    } else if (op == "Add" && stage == 1 && net.dense.size() % 2 == 1) {
      const Initializer* b = nullptr;
      bool on_value = false;
      for (const std::string& in : nd.inputs) {
        if (in == dense_out) on_value = true;
        else b = init_of(m, in);
      }
      Tensor tb;
      if (nd.inputs.size() != 2 || !on_value || !b || b->dims != std::vector<int64_t>{net.dense_cfg.back()} || !floats_of(*b, tb.v))
        refuse(nd, "not the bias of the dense layer before it");
      tb.shape = b->dims;
      net.dense.push_back(std::move(tb));
      dense_out = nd.outputs.empty() ? "" : nd.outputs[0];
    } else {
      refuse(nd, "an operator outside the family, or out of place");
    }
  }
  if (at < n_front) throw FormatError(std::string("not a DNSMOS primary graph: the front end ends before its ") + kFront[at]);
  if (!have_max || net.dense.size() != 6) throw FormatError("not a DNSMOS graph: it needs convolutions, a global maximum and three dense layers with biases");
  if (net.dense_cfg.back() != (primary ? 3 : 1)) throw FormatError(primary ? "not a DNSMOS primary graph: the head must have three outputs" : "not a DNSMOS P.808 graph: the head must have one output");
  if (primary) {
    wr.name = "stft_real"; wi.name = "stft_imag";
    wr.shape = wi.shape = {161, 320};
    net.front = {wr, wi, consts};
  }
}

std::string ints_json(const std::vector<int>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "]";
}

void build(const OnnxModel& primary, const OnnxModel* p808, Container& out) {
  Net nets[2];
  walk(primary, true, nets[0]);
  if (p808) walk(*p808, false, nets[1]);
  const char* const names[2] = {"primary", "p808"};
  std::string tensors;
  size_t off = 0;
  out.blob.clear();
  auto put = [&](const std::string& name, const Tensor& t) {
    std::string shape;
    for (int64_t d : t.shape) shape += (shape.empty() ? "" : ", ") + std::to_string(d);
    tensors += (tensors.empty() ? "" : ", ") + std::string("\"") + name + "\": {\"shape\": [" + shape + "], \"offset\": " + std::to_string(off) + "}";
    const size_t padded = (t.v.size() * 4 + 255) / 256 * 256;
    out.blob.resize((off + padded) / 4, 0.f);
    if (!t.v.empty()) std::memcpy(out.blob.data() + off / 4, t.v.data(), t.v.size() * 4);
    off += padded;
  };
  for (int k = 0; k < (p808 ? 2 : 1); ++k) {
    const std::string pre = std::string(names[k]) + ".";
    for (const Tensor& t : nets[k].front) put(pre + t.name, t);
    for (size_t i = 0; i < nets[k].convs.size(); ++i) put(pre + "conv" + std::to_string(i / 2) + (i % 2 ? ".b" : ".w"), nets[k].convs[i]);
    for (size_t i = 0; i < nets[k].dense.size(); ++i) put(pre + "dense" + std::to_string(i / 2) + (i % 2 ? ".b" : ".w"), nets[k].dense[i]);
  }
  const std::string config = std::string("{\"kind\": \"dnsmos\", \"has_p808\": ") + (p808 ? "1" : "0") + ", \"primary_convs\": " +
                             ints_json(nets[0].conv_cfg) + ", \"primary_dense\": " + ints_json(nets[0].dense_cfg) + ", \"p808_convs\": " +
                             ints_json(nets[1].conv_cfg) + ", \"p808_dense\": " + ints_json(nets[1].dense_cfg) + "}";
  out.manifest = "{\"config\": " + config + ", \"tensors\": {" + tensors + "}, \"total_bytes\": " + std::to_string(off) + "}";
}

}  // namespace

void load_dnsmos_bytes(const void* primary, size_t primary_bytes, const void* p808, size_t p808_bytes, Container& out) {
  out = Container();
  OnnxModel a, b;
  read_onnx_bytes(primary, primary_bytes, a);
  if (p808) read_onnx_bytes(p808, p808_bytes, b);
  build(a, p808 ? &b : nullptr, out);
}

void load_dnsmos(const std::string& primary, const std::string& p808, Container& out) {
  out = Container();
  OnnxModel a, b;
  read_onnx(primary, a);
  if (!p808.empty()) read_onnx(p808, b);
  build(a, p808.empty() ? nullptr : &b, out);
  out.sources = {primary};
  if (!p808.empty()) out.sources.push_back(p808);
}

}  // namespace pfhip_files
