// nrx_model.h -- the model side of libnrx.so's host code (nrx_model.cpp), as the C entry points
// (nrx_api.cpp) use it: topology checks, the weight list, packing + upload, the flop count.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/nrx.h"
#include "nrx_internal.h"

namespace nrx {

// nrx_last_error's message and the code to return (nrx_api.cpp)
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

// Topology checks: the kernels are specialised for the in-scope configs.
int check_desc(const nrx_desc* d);

inline int bits_max(const nrx_desc* d) {
  int b = 0;
  for (int m = 0; m < d->num_mcs; ++m) b = d->bits[m] > b ? d->bits[m] : b;
  return b;
}
// LLR heads = StateInit stages: one with MCS masking, else one per MCS (Var-IO)
inline int num_heads(const nrx_desc* d) { return d->var_mcs_masking ? 1 : d->num_mcs; }
inline int head_bits(const nrx_desc* d, int h) { return d->var_mcs_masking ? bits_max(d) : d->bits[h]; }

// padded StateInit input width (FwdArgs::init_cinp) for MFMA K chunks of kc
int init_padded_cin(const nrx_desc* d, int kc);
// element counts of the weight arrays nrx_create expects, in Keras get_weights() order
std::vector<int64_t> weight_sizes(const nrx_desc* d);
// multiply-adds x 2 per resource element and user of a forward of num_it iterations
double flops_per_re_user(const nrx_desc* d, int num_it);

template <class WT, class BT>
struct DeviceModel {
  ModelW<WT, BT> W{};
  void* dev = nullptr;
  int init_cinp = 0;
};
// pack the weights for MFMA K chunks of kc (32: f16, 16: f64) and upload them
int build_model(const nrx_desc* d, const float* const* w, int kc, DeviceModel<_Float16, float>* out);
int build_model(const nrx_desc* d, const float* const* w, int kc, DeviceModel<double, double>* out);

}  // namespace nrx
