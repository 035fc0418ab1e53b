// nrx_model.cpp -- the model side of libnrx.so's host code: topology checks, the layer list (weight
// sizes, flop count) and the packing of the weights into one device blob per precision.
//
// Weight order = Keras get_weights() of the reference CGNN:
//   StateInit x num_init : 3 x (dw[3,3,Cin,1], pw[1,1,Cin,Cout], b[Cout])
//   num_it x [ Agg: (W[ds,64], b), (W[64,ds], b) ; Update: 3 x sep ]
//   LLR heads x H : (W[ds,128], b), (W[128,bits], b)
//   ChEst : (W[ds,128], b), (W[128,2A], b)
#include "nrx_model.h"

#include <cstring>

namespace nrx {

int check_desc(const nrx_desc* d) {
  if (!d) return fail(NRX_ERR_INVALID_ARG, "desc is NULL");
  if (d->d_s != kDS) return fail(NRX_ERR_UNSUPPORTED, "kernels are built for d_s = 56");
  if (d->init_units[0] != kHID || d->init_units[1] != kHID || d->state_units[0] != kHID ||
      d->state_units[1] != kHID || d->readout_units != kHID || d->agg_units != kAGG)
    return fail(NRX_ERR_UNSUPPORTED, "kernels are built for 128/128 convs, 64 agg, 128 readout");
  if (d->num_rx_ant < 1 || 4 * d->num_rx_ant + 2 > 128 || 2 * d->num_rx_ant > 32)
    return fail(NRX_ERR_UNSUPPORTED, "num_rx_ant must be 1..16");
  if (d->num_it < 1 || d->num_it > kMaxIt) return fail(NRX_ERR_UNSUPPORTED, "num_it must be 1..8");
  if (d->num_mcs < 1 || d->num_mcs > kMaxHeads) return fail(NRX_ERR_UNSUPPORTED, "num_mcs must be 1..8");
  for (int m = 0; m < d->num_mcs; ++m)
    if (d->bits[m] < 1 || d->bits[m] > 8) return fail(NRX_ERR_UNSUPPORTED, "bits must be 1..8");
  if (!d->var_mcs_masking && d->num_mcs > 3)
    return fail(NRX_ERR_UNSUPPORTED, "at most 3 LLR heads (fused readout staging)");
  if (d->use_h_hat != 0 && d->use_h_hat != 1) return fail(NRX_ERR_INVALID_ARG, "use_h_hat must be 0/1");
  return NRX_OK;
}

namespace {

struct LayerShape {
  enum Kind { SEP, DENSE } kind;
  int cin, cout;
};

int init_cin(const nrx_desc* d) { return (d->use_h_hat ? 4 : 2) * d->num_rx_ant + 2; }

// the layers of a forward of num_it iterations, in weight order
std::vector<LayerShape> layer_list(const nrx_desc* d, int num_it) {
  std::vector<LayerShape> L;
  for (int m = 0; m < num_heads(d); ++m) {
    L.push_back({LayerShape::SEP, init_cin(d), kHID});
    L.push_back({LayerShape::SEP, kHID, kHID});
    L.push_back({LayerShape::SEP, kHID, kDS});
  }
  for (int i = 0; i < num_it; ++i) {
    L.push_back({LayerShape::DENSE, kDS, kAGG});
    L.push_back({LayerShape::DENSE, kAGG, kDS});
    L.push_back({LayerShape::SEP, 2 * kDS + 2, kHID});
    L.push_back({LayerShape::SEP, kHID, kHID});
    L.push_back({LayerShape::SEP, kHID, kDS});
  }
  for (int h = 0; h < num_heads(d); ++h) {
    L.push_back({LayerShape::DENSE, kDS, kHID});
    L.push_back({LayerShape::DENSE, kHID, head_bits(d, h)});
  }
  L.push_back({LayerShape::DENSE, kDS, kHID});
  L.push_back({LayerShape::DENSE, kHID, 2 * d->num_rx_ant});
  return L;
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }
int pow2_at_least(int x, int lo) {
  int p = lo;
  while (p < x) p *= 2;
  return p;
}

// Host-side packing into one contiguous blob per precision; pointers are patched to the
// device copy after upload.
template <class WT, class BT>
struct Packer {
  std::vector<char> blob;
  template <class T>
  size_t put(const std::vector<T>& v) {
    size_t off = align256(blob.size());
    blob.resize(off + v.size() * sizeof(T));
    memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
  // offsets relative to blob start, fixed up later
  struct SepOff { size_t dw, pw, b; };
  struct DenOff { size_t w, b; };
  // `pos` (optional) places input channel c at packed position pos[c] (StateInit conv1:
  // the kernel's z image is [y | pe | h] with the antenna blocks padded to A2P).
  SepOff sep(const float* dw, const float* pw, const float* b, int cin, int cout, int cinp, int coutp,
             const std::vector<int>* pos = nullptr) {
    std::vector<WT> dwp((size_t)9 * cinp, WT(0)), pwp((size_t)coutp * cinp, WT(0));
    std::vector<BT> bp(coutp, BT(0));
    auto P = [&](int c) { return pos ? (*pos)[c] : c; };
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < cin; ++c) dwp[(size_t)tap * cinp + P(c)] = (WT)dw[(size_t)tap * cin + c];
    for (int c = 0; c < cin; ++c)
      for (int o = 0; o < cout; ++o) pwp[(size_t)o * cinp + P(c)] = (WT)pw[(size_t)c * cout + o];
    for (int o = 0; o < cout; ++o) bp[o] = (BT)b[o];
    SepOff r;
    r.dw = put(dwp);
    r.pw = put(pwp);
    r.b = put(bp);
    return r;
  }
  // kperm: 0 = natural K order; 32 / 16 = K permuted so that the MFMA C layout of the
  // producing layer (lane (t,g) holds channels 16n + 4g + j (f16) / 16n + g + 4j (f64))
  // is directly the B fragment (kernels: CFrag).
  static int kperm_channel(int p, int kperm) {
    if (kperm == 32) return 32 * (p / 32) + 16 * ((p % 8) / 4) + 4 * ((p % 32) / 8) + (p % 4);
    if (kperm == 16) return 16 * (p / 16) + (p % 16) / 4 + 4 * (p % 4);
    return p;
  }
  DenOff dense(const float* w, const float* b, int cin, int cout, int cinp, int coutp, int kperm = 0) {
    std::vector<WT> wp((size_t)coutp * cinp, WT(0));
    std::vector<BT> bp(coutp, BT(0));
    for (int pk = 0; pk < cinp; ++pk) {
      const int c = kperm_channel(pk, kperm);
      if (c >= cin) continue;
      for (int o = 0; o < cout; ++o) wp[(size_t)o * cinp + pk] = (WT)w[(size_t)c * cout + o];
    }
    for (int o = 0; o < cout; ++o) bp[o] = (BT)b[o];
    DenOff r;
    r.w = put(wp);
    r.b = put(bp);
    return r;
  }
};

template <class WT, class BT>
int build(const nrx_desc* d, const float* const* w, int kc, DeviceModel<WT, BT>* out) {
  Packer<WT, BT> pk;
  using SO = typename Packer<WT, BT>::SepOff;
  using DO = typename Packer<WT, BT>::DenOff;
  SO init[kMaxInit][3];
  DO agg[kMaxIt][2];
  SO upd[kMaxIt][3];
  DO llr[kMaxHeads][2];
  DO ch[2];
  const int icin = init_cin(d);
  // StateInit input z = [y (2A), pe (2), h (2A)] (copy_pytorch.py:175-183) is laid out
  // with each antenna block padded to A2P = init_a2p(A): y at [0, 2A), h at [A2P, A2P+2A),
  // pe at 2 A2P, 2 A2P + 1 (so that an 8-channel lane chunk is all y, all h or pe: the
  // one-launch forward's conv1 loads them straight from y / h_hat / pe); the padded channels
  // carry zero weights.
  const int a2p = init_a2p(d->num_rx_ant);
  std::vector<int> ipos(icin);
  for (int c = 0; c < icin; ++c) {
    const int a2 = 2 * d->num_rx_ant;
    ipos[c] = c < a2 ? c : (c < a2 + 2 ? 2 * a2p + (c - a2) : a2p + (c - a2 - 2));
  }
  const int icinp = init_padded_cin(d, kc);
  out->init_cinp = icinp;
  int k = 0;
  auto sep = [&](int cin, int cout, int cinp, int coutp, const std::vector<int>* pos = nullptr) {
    SO r = pk.sep(w[k], w[k + 1], w[k + 2], cin, cout, cinp, coutp, pos);
    k += 3;
    return r;
  };
  // every dense layer of the engine consumes an MFMA accumulator tile: K permuted
  auto den = [&](int cin, int cout, int cinp, int coutp) {
    DO r = pk.dense(w[k], w[k + 1], cin, cout, cinp, coutp, kc);
    k += 2;
    return r;
  };
  // f16: conv2 / conv3 read the strip image the previous layer's in-place epilogue wrote
  // straight from its accumulators (lane (t, g) stores tiles 2kc, 2kc+1 as one 16-byte
  // chunk 4kc + g), i.e. their input channels sit in the K-permuted order of the dense
  // layers: channel c at packed position kperm^-1(c)
  std::vector<int> hpos(kHID);
  for (int p = 0; p < kHID; ++p) hpos[Packer<WT, BT>::kperm_channel(p, kc == 32 ? 32 : 0)] = p;
  const std::vector<int>* hp = kc == 32 ? &hpos : nullptr;
  for (int m = 0; m < num_heads(d); ++m) {
    init[m][0] = sep(icin, kHID, icinp, kHID, &ipos);
    init[m][1] = sep(kHID, kHID, kHID, kHID, hp);
    init[m][2] = sep(kHID, kDS, kHID, kDSP, hp);
  }
  for (int i = 0; i < d->num_it; ++i) {
    agg[i][0] = den(kDS, kAGG, kDSP, kAGG);
    agg[i][1] = den(kAGG, kDS, kAGG, kDSP);
    upd[i][0] = sep(2 * kDS + 2, kHID, kUPD_CINP, kHID);
    upd[i][1] = sep(kHID, kHID, kHID, kHID, hp);
    upd[i][2] = sep(kHID, kDS, kHID, kDSP, hp);
  }
  for (int h = 0; h < num_heads(d); ++h) {
    llr[h][0] = den(kDS, kHID, kDSP, kHID);
    llr[h][1] = den(kHID, head_bits(d, h), kHID, 16);
  }
  const int a2 = 2 * d->num_rx_ant;
  ch[0] = den(kDS, kHID, kDSP, kHID);
  ch[1] = den(kHID, a2, kHID, a2 <= 16 ? 16 : 32);

  hipError_t e = hipMalloc(&out->dev, pk.blob.size());
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(weights)");
  e = hipMemcpy(out->dev, pk.blob.data(), pk.blob.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy(weights)");
  char* base = (char*)out->dev;
  auto fs = [&](const SO& o) {
    return SepW<WT, BT>{(const WT*)(base + o.dw), (const WT*)(base + o.pw), (const BT*)(base + o.b)};
  };
  auto fd = [&](const DO& o) { return DenseW<WT, BT>{(const WT*)(base + o.w), (const BT*)(base + o.b)}; };
  for (int m = 0; m < num_heads(d); ++m)
    for (int l = 0; l < 3; ++l) out->W.init[m][l] = fs(init[m][l]);
  for (int i = 0; i < d->num_it; ++i) {
    out->W.agg[i][0] = fd(agg[i][0]);
    out->W.agg[i][1] = fd(agg[i][1]);
    for (int l = 0; l < 3; ++l) out->W.upd[i][l] = fs(upd[i][l]);
  }
  for (int h = 0; h < num_heads(d); ++h) {
    out->W.llr[h][0] = fd(llr[h][0]);
    out->W.llr[h][1] = fd(llr[h][1]);
  }
  out->W.chest[0] = fd(ch[0]);
  out->W.chest[1] = fd(ch[1]);
  return NRX_OK;
}

}  // namespace

int init_padded_cin(const nrx_desc* d, int kc) {
  return pow2_at_least(round_up(2 * init_a2p(d->num_rx_ant) + 2, kc), 32);
}

std::vector<int64_t> weight_sizes(const nrx_desc* d) {
  std::vector<int64_t> s;
  for (const auto& l : layer_list(d, d->num_it)) {
    if (l.kind == LayerShape::SEP) s.push_back(9LL * l.cin);
    s.push_back((int64_t)l.cin * l.cout);
    s.push_back(l.cout);
  }
  return s;
}

double flops_per_re_user(const nrx_desc* d, int num_it) {
  auto macs = [&](int it) {   // biases are not counted
    int64_t n = 0;
    for (const auto& l : layer_list(d, it)) n += (l.kind == LayerShape::SEP ? 9LL * l.cin : 0) + (int64_t)l.cin * l.cout;
    return n;
  };
  const int64_t fixed = macs(0), per_it = macs(1) - fixed;   // integers: exact in double
  return 2.0 * ((double)fixed + (double)num_it * (double)per_it);
}

int build_model(const nrx_desc* d, const float* const* w, int kc, DeviceModel<_Float16, float>* out) {
  return build(d, w, kc, out);
}
int build_model(const nrx_desc* d, const float* const* w, int kc, DeviceModel<double, double>* out) {
  return build(d, w, kc, out);
}

}  // namespace nrx
