// nrx_api.cpp -- the C ABI of libnrx.so (include/nrx.h): the argument checks the entry points share,
// workspace sizing, forward dispatch, and the product-side positional encoding.  The model side
// (topology checks, weight packing, flop count) is nrx_model.cpp.
//
// An entry point checks its descriptor first (check_grid, check_mcs_bits, ... below), then the
// handle and the workspace pointer and alignment, then the workspace size (check_workspace), all
// before its first HIP call, and ends in launched().
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nrx.h"
#include "nrx_internal.h"
#include "nrx_model.h"

namespace nrx {
hipError_t launch_forward_f16(const FwdArgs<_Float16, float, _Float16>& args, const ModelW<_Float16, float>& W,
                              const FwdPlan& pl, const FusedCtl& fc, hipStream_t st, Prof* prof);
void device_counts(int* cus, int* xccs);
size_t fused_sync_bytes();
hipError_t fused_sync_status(void* sync, int* st, bool reset, hipEvent_t last);
hipError_t run_tier_p64(const FwdArgs<double, double, float>& args, const ModelW<double, double>& W,
                        const FwdPlan& pl, hipStream_t st, Prof* prof);
hipError_t setup_kernels();
int strip_width(int precision);

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(NRX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace nrx

using namespace nrx;

// ---------------------------------------------------------------- shared argument checks
// One rule has one wording and one code wherever it applies; what differs between entry points on
// purpose is an argument at the call site.
namespace {

int check_range(const char* name, long v, long lo, long hi, int code = NRX_ERR_SHAPE) {
  if (v >= lo && v <= hi) return NRX_OK;
  return fail(code, std::string(name) + " must be " + std::to_string(lo) + ".." + std::to_string(hi));
}

// The slot grid [batch][num_tx][num_subcarriers][14].  tx_supported: the detectors' kernels stop at 8
// users, which is NRX_ERR_UNSUPPORTED, not a bad shape; min_subcarriers: the generator's pilot comb
// needs 2.
template <class IO>
int check_grid(const IO* io, int tx_supported = kMaxUsers, int min_subcarriers = 1) {
  if (io->num_symbols != kT) return fail(NRX_ERR_SHAPE, "num_symbols must be 14");
  if (int rc = check_range("batch", io->batch, 1, 65535)) return rc;
  if (int rc = check_range("num_subcarriers", io->num_subcarriers, min_subcarriers, 12 * 275)) return rc;
  if (io->num_tx > tx_supported && tx_supported < kMaxUsers)
    return fail(NRX_ERR_UNSUPPORTED, "the kernels are built for num_tx <= " + std::to_string(tx_supported));
  return check_range("num_tx", io->num_tx, 1, kMaxUsers);
}
// ... with receive antennas
template <class IO>
int check_grid_ant(const IO* io, int tx_supported = kMaxUsers, int min_subcarriers = 1) {
  if (int rc = check_grid(io, tx_supported, min_subcarriers)) return rc;
  return check_range("num_rx_ant", io->num_rx_ant, 1, 16);
}

// num_mcs 1..8 (num_mcs_code: the generator reports it as a bad argument, the others as a bad shape)
// and every mcs_bits[m] a QAM order the detectors and the generator know (qam: 2, 4 or 6) or 1..8
int check_mcs_bits(const int32_t* bits, int num_mcs, bool qam, int num_mcs_code = NRX_ERR_SHAPE) {
  if (int rc = check_range("num_mcs", num_mcs, 1, 8, num_mcs_code)) return rc;
  for (int m = 0; m < num_mcs; ++m)
    if (qam ? bits[m] != 2 && bits[m] != 4 && bits[m] != 6 : bits[m] < 1 || bits[m] > 8)
      return fail(NRX_ERR_INVALID_ARG, qam ? "mcs_bits must be 2, 4 or 6" : "mcs_bits must be 1..8");
  return NRX_OK;
}
// the bit axis of an LLR / bit tensor holds the widest MCS (after check_mcs_bits)
int check_bits_stride(int bits_stride, const int32_t* bits, int num_mcs) {
  for (int m = 0; m < num_mcs; ++m)
    if (bits_stride < bits[m]) return fail(NRX_ERR_SHAPE, "bits_stride < max(mcs_bits)");
  return NRX_OK;
}

// 1..4 ascending DMRS symbols; *mask (optional): their bit mask
int check_dmrs_symbols(const int32_t* sym, int n, int* mask = nullptr) {
  if (int rc = check_range("num_dmrs_symbols", n, 1, 4)) return rc;
  int bits = 0;
  for (int k = 0; k < n; ++k) {
    if (sym[k] < 0 || sym[k] >= kT || (k && sym[k] <= sym[k - 1]))
      return fail(NRX_ERR_INVALID_ARG, "dmrs_symbols must be ascending symbol indices below 14");
    bits |= 1 << sym[k];
  }
  if (mask) *mask = bits;
  return NRX_OK;
}
int check_cdm_group(const int32_t* group, int num_tx) {
  for (int u = 0; u < num_tx; ++u)
    if (group[u] != 0 && group[u] != 1) return fail(NRX_ERR_INVALID_ARG, "cdm_group must be 0/1");
  return NRX_OK;
}
// Cover-coded DMRS ports (nrx_ls_estimate, nrx_generate_slots_dmrs), after check_grid, check_dmrs_symbols and
// check_cdm_group: covers and despreading flags 0/1, every port < num_tx its own (group, focc, tocc), a cover
// only with its despreading, and the grid in whole despreading blocks
int check_dmrs_ports(int num_tx, const int32_t* group, const int32_t* focc, const int32_t* tocc, int despread_f,
                     int despread_t, int num_subcarriers, const int32_t* sym, int num_dmrs_symbols) {
  if (int rc = check_range("despread_f", despread_f, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_range("despread_t", despread_t, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  unsigned seen = 0;
  for (int u = 0; u < num_tx; ++u) {
    if ((focc[u] != 0 && focc[u] != 1) || (tocc[u] != 0 && tocc[u] != 1))
      return fail(NRX_ERR_INVALID_ARG, "focc and tocc must be 0/1");
    const unsigned bit = 1u << (group[u] + 2 * focc[u] + 4 * tocc[u]);
    if (seen & bit) return fail(NRX_ERR_INVALID_ARG, "two ports share one (cdm_group, focc, tocc)");
    seen |= bit;
    if (focc[u] && !despread_f) return fail(NRX_ERR_INVALID_ARG, "a port with focc = 1 needs despread_f");
    if (tocc[u] && !despread_t) return fail(NRX_ERR_INVALID_ARG, "a port with tocc = 1 needs despread_t");
  }
  if (despread_f && num_subcarriers % 4)
    return fail(NRX_ERR_SHAPE, "despread_f needs num_subcarriers % 4 == 0 (pairs of comb positions)");
  if (despread_t) {
    bool ok = num_dmrs_symbols % 2 == 0;
    for (int k = 0; ok && k < num_dmrs_symbols; k += 2) ok = sym[k + 1] == sym[k] + 1;
    if (!ok) return fail(NRX_ERR_INVALID_ARG, "despread_t needs dmrs_symbols in pairs (t, t + 1)");
  }
  return NRX_OK;
}
int check_aerial_list(const void* re, const void* im, int num_subcarriers) {
  if ((re == nullptr) != (im == nullptr)) return fail(NRX_ERR_INVALID_ARG, "Aerial outputs come in (real, imag) pairs");
  if (re && num_subcarriers % 12) return fail(NRX_ERR_SHAPE, "Aerial pilot list needs num_subcarriers % 12 == 0");
  return NRX_OK;
}
int check_symbol_mask(const char* name, int v) {
  if (v >= 0 && v < (1 << kT)) return NRX_OK;
  return fail(NRX_ERR_INVALID_ARG, std::string(name) + " must be a mask of the 14 symbols");
}
int check_pos(const char* name, double v) {
  if (v > 0.0 && std::isfinite(v)) return NRX_OK;
  return fail(NRX_ERR_INVALID_ARG, std::string(name) + " must be finite and > 0");
}
int check_nonneg(const char* name, double v) {
  if (v >= 0.0 && std::isfinite(v)) return NRX_OK;
  return fail(NRX_ERR_INVALID_ARG, std::string(name) + " must be finite and >= 0");
}

// the taps l_min..l_max of the time-domain channel (nrx_tc_io, nrx_gen_tc)
int check_tap_span(long l_min, long l_max) {
  if (int rc = check_range("l_min", l_min, -255, 0)) return rc;
  if (int rc = check_range("l_max", l_max, 0, 255)) return rc;
  if (l_max - l_min + 1 > 256) return fail(NRX_ERR_SHAPE, "the tap span l_max - l_min + 1 must be <= 256");
  return NRX_OK;
}

int too_small(size_t need) {
  return fail(NRX_ERR_WORKSPACE, "workspace too small: need " + std::to_string(need) + " bytes");
}
// The workspace of a launch, after its descriptor checks: the pointer, the alignment of the kernels'
// widest access to it (1: none), then the size.
int check_workspace(const void* ws, size_t bytes, size_t need, size_t align) {
  if (!ws) return fail(NRX_ERR_INVALID_ARG, "null workspace pointer");
  if ((uintptr_t)ws & (align - 1))
    return fail(NRX_ERR_INVALID_ARG, "workspace must be " + std::to_string(align) + "-byte aligned");
  return bytes < need ? too_small(need) : NRX_OK;
}
// the end of a *_workspace_size call, after its descriptor checks
int store_size(size_t* bytes, size_t need) {
  if (!bytes) return fail(NRX_ERR_INVALID_ARG, "bytes is NULL");
  *bytes = need;
  return NRX_OK;
}
// the end of a launching call
int launched(hipError_t e, const char* what) { return e == hipSuccess ? NRX_OK : hip_fail(e, what); }

}  // namespace

// Event-pair recorder behind nrx_profile_enable / nrx_profile_read.
struct EventProf : Prof {
  struct Rec { int kid; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  void begin(int kid, void* st) override {
    Rec r{kid, get(), nullptr};
    (void)hipEventRecord(r.a, (hipStream_t)st);
    recs.push_back(r);
  }
  void end(int, void* st) override {
    hipEvent_t e = get();
    (void)hipEventRecord(e, (hipStream_t)st);
    recs.back().b = e;
  }
  // fold finished records into totals
  int64_t launches[K_COUNT] = {0};
  double total_ms[K_COUNT] = {0};
  hipError_t collect() {
    for (auto& r : recs) {
      hipError_t e = hipEventSynchronize(r.b);
      if (e != hipSuccess) return e;
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, r.a, r.b);
      if (e != hipSuccess) return e;
      launches[r.kid] += 1;
      total_ms[r.kid] += ms;
      pool.push_back(r.a);
      pool.push_back(r.b);
    }
    recs.clear();
    return hipSuccess;
  }
  void reset() {
    for (int k = 0; k < K_COUNT; ++k) {
      launches[k] = 0;
      total_ms[k] = 0;
    }
  }
  ~EventProf() override {
    for (auto& r : recs) {
      (void)hipEventDestroy(r.a);
      if (r.b) (void)hipEventDestroy(r.b);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

struct nrx_handle {
  nrx_desc desc;
  int device;
  DeviceModel<_Float16, float> m16;
  DeviceModel<double, double> m64;
  EventProf* prof = nullptr;
  void* fused_sync = nullptr;   // k_forward's work queues and dependency counters (zeroed)
  int fused_enabled = 1;    // NRX_FUSED (environment, read once at nrx_create)
  int spin_limit = kFusedSpinLimit;
  int dbg_err = 0;
  int update_rr = kSchedDefault;   // nrx_update_schedule (NRX_UPDATE_RR at nrx_create)
  // one-stream rule of the one-launch forward: an event the handle owns, recorded
  // behind every eager one-launch forward, stands for "that forward is done" -- the caller's
  // stream itself is never kept (it may be destroyed between calls).  last_stream is compared,
  // never used.  Forwards captured into a hipGraph record no event: graph replays are outside
  // the guard (the caller keeps replays of one handle on one stream).
  hipEvent_t last_ev = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  FusedCtl fused_ctl() const { return FusedCtl{fused_sync, spin_limit, dbg_err}; }
  int small_tiers = 1;      // nrx_debug_small_tiers (tests)
  Sched sched() const { return Sched{update_rr, fused_enabled, small_tiers}; }
};

// The forward workspace: the slot norms, four state / aggregate planes [B][U][F][14][56] of the storage type
// (_Float16 or float) and, in f16 workspaces only, the pe16 plane [U][F][14][56] of the one-launch forward.
// ws == nullptr: the size query.
struct FwdWs {
  double* norm;
  void *s_out, *s_in, *a_out, *a, *pe16;
  size_t total;
};
static FwdWs fwd_layout(const nrx_shape* s, int precision, void* ws) {
  const bool f16 = precision == NRX_PREC_F16;
  const size_t plane = (size_t)s->num_tx * s->num_subcarriers * kT * kDS * (f16 ? 2 : 4);
  Carver c(ws);
  FwdWs w{};
  w.norm = c.take<double>(s->batch);
  w.s_out = c.take<char>(s->batch * plane);
  w.s_in = c.take<char>(s->batch * plane);
  w.a_out = c.take<char>(s->batch * plane);
  w.a = c.take<char>(s->batch * plane);
  if (f16) w.pe16 = c.take<char>(plane);
  w.total = c.bytes();
  return w;
}
static size_t ws_bytes_of(const nrx_shape* s, int precision) { return fwd_layout(s, precision, nullptr).total; }

static int check_shape(const nrx_shape* s) {
  if (!s) return fail(NRX_ERR_INVALID_ARG, "shape is NULL");
  return check_grid(s);
}

template <class WT, class BT, class S>
static void fill_args(FwdArgs<WT, BT, S>& a, const nrx_desc* d, const nrx_io* io, void* ws, int init_cinp) {
  const nrx_shape* s = &io->shape;
  a.B = s->batch;
  a.llr_B = s->batch;
  a.U = s->num_tx;
  a.F = s->num_subcarriers;
  a.A = d->num_rx_ant;
  a.M = d->num_mcs;
  a.H = num_heads(d);
  a.init_cinp = init_cinp;
  a.num_init = num_heads(d);
  a.masking = d->var_mcs_masking;
  a.use_h = d->use_h_hat;
  a.bits_max = bits_max(d);
  for (int i = 0; i < kMaxHeads; ++i)
    a.head_bits[i] = i < a.H ? head_bits(d, i) : 0;
  a.y = io->y;
  a.pe = io->pe;
  a.h_hat = io->h_hat;
  a.active = io->active;
  a.mcs_mask = io->mcs_mask;
  a.llr = io->llr;
  a.h_ref = io->h_ref;
  const FwdWs w = fwd_layout(s, io->precision, ws);
  a.norm = w.norm;
  a.s_in = (S*)w.s_in;
  a.s_out = (S*)w.s_out;
  a.a = (S*)w.a;
  a.a_out = (S*)w.a_out;
  a.pe16 = (S*)w.pe16;
  a.ws_base = (const char*)ws;
  a.ws_bytes = w.total < 0xFFFFFFFFull ? (unsigned)w.total : 0xFFFFFFFFu;
}

static int forward_slots(nrx_handle* h, const nrx_io* io, int llr_B, void* workspace, hipStream_t st);
static int chunk_slots(const nrx_shape* s, int precision);

// The slot chunks [b0, b0 + n) a forward of s->batch slots runs as (chunk_slots): f(b0, n) each, until one fails.
template <class F>
static int each_chunk(const nrx_shape* s, int precision, F f) {
  const int B = s->batch, bc = chunk_slots(s, precision);
  for (int b0 = 0; b0 < B; b0 += bc)
    if (int rc = f(b0, b0 + bc < B ? bc : B - b0)) return rc;
  return NRX_OK;
}

// The plan of an f16 forward over n slots of io's shape in workspace ws (never null: pe16 gates the GZ paths); fills a.
static FwdPlan plan_f16(FwdArgs<_Float16, float, _Float16>& a, const nrx_desc* d, const nrx_io* io, int n, void* ws,
                        int init_cinp, const Sched& sc, int cus, int xccs) {
  nrx_io c = *io;
  c.shape.batch = n;
  fill_args(a, d, &c, ws, init_cinp);
  return plan_forward(a, io->num_it, sc, cus, xccs);
}

// The one-stream rule: NRX_ERR_BUSY when a forward that takes the one-launch path arrives on a stream
// other than the previous one-launch forward's while that forward has not finished (the counters are
// per handle).
static int busy(const nrx_handle* h, hipStream_t st) {
  if (h->have_last && h->last_stream != st && hipEventQuery(h->last_ev) == hipErrorNotReady)
    return fail(NRX_ERR_BUSY, "a one-launch forward of this handle is still running on another stream");
  return NRX_OK;
}

// busy() for the whole of a forward entry point, called before ANY of its launches, so a refused
// call has launched nothing (the y-layout / Aerial preprocessing used to run first).
// Decided on the shapes the forward will run: each slot chunk may take the one-launch path although the
// whole batch would not; one plan per distinct chunk size.
static int fused_busy(nrx_handle* h, const nrx_io* io, void* ws, hipStream_t st) {
  if (io->precision != NRX_PREC_F16) return NRX_OK;
  int cus, xccs, seen = 0;
  device_counts(&cus, &xccs);
  bool takes = false;
  (void)each_chunk(&io->shape, io->precision, [&](int, int n) {
    FwdArgs<_Float16, float, _Float16> a{};
    takes = takes ||
            (n != seen && plan_f16(a, &h->desc, io, n, ws, h->m16.init_cinp, h->sched(), cus, xccs).one_launch());
    seen = n;
    return 0;
  });
  return takes ? busy(h, st) : NRX_OK;
}

extern "C" {

const char* nrx_last_error(void) { return g_err.c_str(); }
int32_t nrx_api_version(void) { return NRX_API_VERSION; }

int nrx_weight_layout(const nrx_desc* desc, int32_t* num_weights, int64_t* sizes, int32_t cap) {
  if (int rc = check_desc(desc)) return rc;
  if (!num_weights) return fail(NRX_ERR_INVALID_ARG, "num_weights is NULL");
  std::vector<int64_t> s = weight_sizes(desc);
  *num_weights = (int32_t)s.size();
  if (sizes)
    for (int i = 0; i < (int)s.size() && i < cap; ++i) sizes[i] = s[i];
  return NRX_OK;
}

int nrx_create(const nrx_desc* desc, const float* const* weights, const int64_t* sizes,
               int32_t num_weights, int32_t device, nrx_handle** out) {
  int rc = check_desc(desc);
  if (rc) return rc;
  if (!weights || !sizes || !out) return fail(NRX_ERR_INVALID_ARG, "null argument");
  std::vector<int64_t> exp = weight_sizes(desc);
  if ((int)exp.size() != num_weights)
    return fail(NRX_ERR_SHAPE, "expected " + std::to_string(exp.size()) + " weight arrays, got " +
                                   std::to_string(num_weights));
  for (int i = 0; i < num_weights; ++i) {
    if (!weights[i]) return fail(NRX_ERR_INVALID_ARG, "weight " + std::to_string(i) + " is NULL");
    if (sizes[i] != exp[i])
      return fail(NRX_ERR_SHAPE, "weight " + std::to_string(i) + " has " + std::to_string(sizes[i]) +
                                     " elements, expected " + std::to_string(exp[i]));
  }
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  e = setup_kernels();
  if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute");
  nrx_handle* h = new nrx_handle();
  h->desc = *desc;
  h->device = device;
  {
    // A/B and bit-identity tests: 0 = three launches, 1 = default, 2 (or "force") = wherever it
    // applies; anything else is rejected rather than silently read as 0
    const char* ev = getenv("NRX_FUSED");
    if (ev && *ev) {
      if (!strcmp(ev, "0") || !strcmp(ev, "off")) h->fused_enabled = 0;
      else if (!strcmp(ev, "1") || !strcmp(ev, "on")) h->fused_enabled = 1;
      else if (!strcmp(ev, "2") || !strcmp(ev, "force")) h->fused_enabled = 2;
      else {
        delete h;
        return fail(NRX_ERR_INVALID_ARG, std::string("NRX_FUSED must be 0/off, 1/on or 2/force, got '") + ev + "'");
      }
    }
  }
  {
    const char* ev = getenv("NRX_UPDATE_RR");   // A/B: 0 = strip update kernels
    if (ev && *ev) {
      char* end = nullptr;
      const long v = strtol(ev, &end, 10);
      if (end && !*end && ev[0] >= '0' && ev[0] <= '9' && v >= 0 && v <= kSchedMax) h->update_rr = (int)v;
      else {
        delete h;
        return fail(NRX_ERR_INVALID_ARG, std::string("NRX_UPDATE_RR must be a stage mask 0..127, got '") + ev + "'");
      }
    }
  }
  e = hipMalloc(&h->fused_sync, fused_sync_bytes());
  if (e == hipSuccess) e = hipMemset(h->fused_sync, 0, fused_sync_bytes());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->last_ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    nrx_destroy(h);
    return hip_fail(e, "fused forward counters");
  }
  rc = build_model(desc, weights, 32, &h->m16);
  if (!rc) rc = build_model(desc, weights, 16, &h->m64);
  if (rc) {
    nrx_destroy(h);
    return rc;
  }
  *out = h;
  return NRX_OK;
}

void nrx_destroy(nrx_handle* h) {
  if (!h) return;
  if (h->m16.dev) (void)hipFree(h->m16.dev);
  if (h->m64.dev) (void)hipFree(h->m64.dev);
  if (h->fused_sync) (void)hipFree(h->fused_sync);
  if (h->last_ev) (void)hipEventDestroy(h->last_ev);
  delete h->prof;
  delete h;
}

// Slots per sub-forward.  An f16 forward whose workspace would reach kGzRange runs as
// consecutive forwards of at most this many slots on the caller's stream (slots are independent,
// neural_rx.py:544-595 has no cross-slot term), each in the same workspace: conv1's z-row loader
// then always addresses it with 32-bit buffer offsets, and the workspace shrinks to one chunk's.
static int chunk_slots(const nrx_shape* s, int precision) {
  if (precision != NRX_PREC_F16 || ws_bytes_of(s, precision) < kGzRange) return s->batch;
  int lo = 1, hi = s->batch - 1;   // the largest chunk below the range (one slot always fits: F <= 3300)
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    nrx_shape c = *s;
    c.batch = mid;
    if (ws_bytes_of(&c, precision) < kGzRange) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

int nrx_workspace_size(const nrx_handle* h, const nrx_shape* shape, int32_t precision, size_t* bytes) {
  if (!h || !bytes) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (int rc = check_shape(shape)) return rc;
  if (precision != NRX_PREC_F16 && precision != NRX_PREC_F32X)
    return fail(NRX_ERR_INVALID_ARG, "unknown precision");
  nrx_shape c = *shape;
  c.batch = chunk_slots(shape, precision);
  *bytes = ws_bytes_of(&c, precision);
  return NRX_OK;
}

int nrx_forward(nrx_handle* h, const nrx_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !io) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (int rc = check_shape(&io->shape)) return rc;
  const nrx_desc* d = &h->desc;
  if (io->num_it < 1 || io->num_it > d->num_it) return fail(NRX_ERR_INVALID_ARG, "Invalid number of iterations");
  if (!io->y || !io->pe || !io->active || !io->llr) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (d->use_h_hat && !io->h_hat) return fail(NRX_ERR_INVALID_ARG, "h_hat is required by this model");
  size_t need = 0;
  if (int rc = nrx_workspace_size(h, &io->shape, io->precision, &need)) return rc;
  if (!workspace || workspace_bytes < need) return too_small(need);
  hipStream_t st = (hipStream_t)stream;
  // slot chunks (chunk_slots): the same forward on [b0, b0 + n) with offset tensors; the LLR tensor keeps its
  // head stride (llr_B)
  const int U = io->shape.num_tx, A2 = 2 * d->num_rx_ant;
  const size_t re = (size_t)io->shape.num_subcarriers * kT;
  return each_chunk(&io->shape, io->precision, [&](int b0, int n) {
    nrx_io c = *io;
    c.shape.batch = n;
    c.y = io->y + (size_t)b0 * re * A2;
    c.h_hat = io->h_hat ? io->h_hat + (size_t)b0 * U * re * A2 : nullptr;
    c.active = io->active + (size_t)b0 * U;
    c.mcs_mask = io->mcs_mask ? io->mcs_mask + (size_t)b0 * U * d->num_mcs : nullptr;
    c.h_ref = io->h_ref ? io->h_ref + (size_t)b0 * U * re * A2 : nullptr;
    c.llr = io->llr + (size_t)b0 * U * re * bits_max(d);
    return forward_slots(h, &c, io->shape.batch, workspace, st);
  });
}

// One forward over io->shape.batch slots of an LLR tensor of llr_B slots (its head stride), by one plan.
static int forward_slots(nrx_handle* h, const nrx_io* io, int llr_B, void* workspace, hipStream_t st) {
  hipError_t e;
  if (io->precision == NRX_PREC_F16) {
    int cus, xccs;
    device_counts(&cus, &xccs);
    FwdArgs<_Float16, float, _Float16> a{};
    const FwdPlan pl = plan_f16(a, &h->desc, io, io->shape.batch, workspace, h->m16.init_cinp, h->sched(), cus, xccs);
    a.llr_B = llr_B;
    if (pl.one_launch())
      if (int rc = busy(h, st)) return rc;
    e = launch_forward_f16(a, h->m16.W, pl, h->fused_ctl(), st, h->prof);
    if (e == hipSuccess && pl.one_launch()) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
        e = hipEventRecord(h->last_ev, st);
        h->last_stream = st;
        h->have_last = e == hipSuccess;
      }
    }
  } else {
    FwdArgs<double, double, float> a{};
    fill_args(a, &h->desc, io, workspace, h->m64.init_cinp);
    a.llr_B = llr_B;
    e = run_tier_p64(a, h->m64.W, plan_forward(a, io->num_it), st, h->prof);
  }
  return launched(e, "kernel launch");
}

// y in the CGNN layout [B][F][T][2A], the block of a forward_ex workspace in front of the forward's own
static float* take_y_cgnn(Carver& c, const nrx_handle* h, const nrx_shape* s) {
  return c.take<float>((size_t)s->batch * s->num_subcarriers * s->num_symbols * 2 * h->desc.num_rx_ant);
}

int nrx_workspace_size_ex(const nrx_handle* h, const nrx_shape* shape, int32_t precision, int32_t y_layout,
                          size_t* bytes) {
  if (int rc = nrx_workspace_size(h, shape, precision, bytes)) return rc;
  if (y_layout < NRX_Y_CGNN || y_layout > NRX_Y_SPLIT) return fail(NRX_ERR_INVALID_ARG, "unknown y layout");
  Carver c(nullptr);
  if (y_layout != NRX_Y_CGNN) take_y_cgnn(c, h, shape);
  *bytes += c.bytes();
  return NRX_OK;
}

int nrx_forward_ex(nrx_handle* h, const nrx_io* io, int32_t y_layout, const float* y_imag, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!h || !io) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (y_layout == NRX_Y_CGNN) {
    if (y_imag) return fail(NRX_ERR_INVALID_ARG, "y_imag is only used with NRX_Y_SPLIT");
    return nrx_forward(h, io, workspace, workspace_bytes, stream);
  }
  size_t need = 0;
  if (int rc = nrx_workspace_size_ex(h, &io->shape, io->precision, y_layout, &need)) return rc;
  if (!workspace || workspace_bytes < need) return too_small(need);
  if (!io->y || ((y_layout == NRX_Y_SPLIT) != (y_imag != nullptr)))
    return fail(NRX_ERR_INVALID_ARG, "y / y_imag do not match the y layout");
  Carver c(workspace);
  float* ycg = take_y_cgnn(c, h, &io->shape);
  const size_t fwd_bytes = workspace_bytes - c.bytes();   // the rest is the forward's
  void* fwd_ws = c.take<char>(fwd_bytes);
  if (int rc = fused_busy(h, io, fwd_ws, (hipStream_t)stream)) return rc;
  hipError_t e = launch_y_layout(io->y, y_imag, y_layout, io->shape.batch, io->shape.num_subcarriers,
                                 io->shape.num_symbols, h->desc.num_rx_ant, ycg, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "y layout launch");
  nrx_io cio = *io;
  cio.y = ycg;
  return nrx_forward(h, &cio, fwd_ws, fwd_bytes, stream);
}

// ---------------------------------------------------------------- Aerial contract
namespace {
struct AerialWs {
  float* y;
  float* h;
  float* pe;
  int32_t* nn;
  float* llr;
  void* cgnn;
  size_t cgnn_bytes;
  size_t total;
};

AerialWs aerial_layout(const nrx_handle* h, const nrx_aerial_io* io, void* base, size_t cgnn_bytes) {
  const nrx_shape& s = io->shape;
  const size_t A2 = 2 * (size_t)h->desc.num_rx_ant;
  const size_t re = (size_t)s.num_subcarriers * s.num_symbols;
  AerialWs w{};
  Carver c(base);
  w.y = c.take<float>((size_t)s.batch * re * A2);
  w.h = c.take<float>((size_t)s.batch * s.num_tx * re * A2);
  w.pe = c.take<float>((size_t)s.num_tx * re * 2);
  w.nn = c.take<int32_t>((size_t)s.num_tx * s.num_symbols * 12);
  w.llr = c.take<float>((size_t)num_heads(&h->desc) * s.batch * s.num_tx * re * bits_max(&h->desc));
  w.cgnn = c.take<char>(cgnn_bytes);
  w.cgnn_bytes = cgnn_bytes;
  w.total = c.bytes();
  return w;
}

int check_aerial(const nrx_handle* h, const nrx_aerial_io* io) {
  if (!h || !io) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (int rc = check_shape(&io->shape)) return rc;
  if (io->shape.num_subcarriers % 12) return fail(NRX_ERR_SHAPE, "num_subcarriers must be a multiple of 12 (PRBs)");
  if (int rc = check_range("num_dmrs_symbols", io->num_dmrs_symbols, 1, 14)) return rc;
  if (io->num_dmrs_subcarriers < 2 || io->num_dmrs_subcarriers > 12 || io->num_dmrs_subcarriers % 2)
    return fail(NRX_ERR_SHAPE, "num_dmrs_subcarriers must be even and 2..12 (FOCC pairs)");
  return NRX_OK;
}

// The two preprocessing launches of the Aerial contract (NN table + PE, then y and h_hat), shared
// by nrx_forward_aerial and nrx_aerial_preprocess so that both run the same code on the same
// arguments.
hipError_t aerial_prepare(const nrx_handle* h, const nrx_aerial_io* io, float* y, float* h_hat, float* pe,
                          int32_t* nn, hipStream_t st) {
  const nrx_shape& s = io->shape;
  hipError_t e = launch_aerial_tables(io->dmrs_ofdm_pos, io->dmrs_subcarrier_pos, s.num_tx, io->num_dmrs_symbols,
                                      io->num_dmrs_subcarriers, s.num_symbols, s.num_subcarriers, nn, pe, st);
  if (e == hipSuccess)
    e = launch_aerial_inputs(io->y_real, io->y_imag, io->h_ls_real, io->h_ls_imag, nn, s.batch, s.num_tx,
                             s.num_subcarriers, s.num_symbols, h->desc.num_rx_ant, io->num_dmrs_symbols,
                             io->num_dmrs_subcarriers, y, h_hat, st);
  return e;
}
}  // namespace

int nrx_aerial_preprocess(const nrx_handle* h, const nrx_aerial_io* io, float* y, float* h_hat, float* pe,
                          int32_t* nn, void* stream) {
  if (int rc = check_aerial(h, io)) return rc;
  if (!io->y_real || !io->y_imag || !io->h_ls_real || !io->h_ls_imag || !io->dmrs_ofdm_pos ||
      !io->dmrs_subcarrier_pos)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (!y || !h_hat || !pe || !nn) return fail(NRX_ERR_INVALID_ARG, "null output pointer");
  return launched(aerial_prepare(h, io, y, h_hat, pe, nn, (hipStream_t)stream), "aerial preprocessing launch");
}

int nrx_aerial_workspace_size(const nrx_handle* h, const nrx_aerial_io* io, size_t* bytes) {
  if (int rc = check_aerial(h, io)) return rc;
  if (!bytes) return fail(NRX_ERR_INVALID_ARG, "null argument");
  size_t cg = 0;
  if (int rc = nrx_workspace_size(h, &io->shape, io->precision, &cg)) return rc;
  *bytes = aerial_layout(h, io, nullptr, cg).total;
  return NRX_OK;
}

int nrx_forward_aerial(nrx_handle* h, const nrx_aerial_io* io, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (int rc = check_aerial(h, io)) return rc;
  if (!io->y_real || !io->y_imag || !io->h_ls_real || !io->h_ls_imag || !io->dmrs_port_mask ||
      !io->dmrs_ofdm_pos || !io->dmrs_subcarrier_pos || !io->llr)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  size_t cg = 0;
  if (int rc = nrx_workspace_size(h, &io->shape, io->precision, &cg)) return rc;
  const AerialWs w = aerial_layout(h, io, workspace, cg);
  if (!workspace || workspace_bytes < w.total) return too_small(w.total);
  const nrx_shape& s = io->shape;
  hipStream_t st = (hipStream_t)stream;
  nrx_io cio{};   // the CGNN forward on the preprocessed tensors (mcs_mask NULL)
  cio.shape = s;
  cio.num_it = io->num_it;
  cio.precision = io->precision;
  cio.y = w.y;
  cio.pe = w.pe;
  cio.h_hat = w.h;
  cio.active = io->dmrs_port_mask;
  cio.llr = w.llr;
  cio.h_ref = io->h_hat;
  if (int rc = fused_busy(h, &cio, w.cgnn, st)) return rc;
  hipError_t e = aerial_prepare(h, io, w.y, w.h, w.pe, w.nn, st);
  if (e != hipSuccess) return hip_fail(e, "aerial preprocessing launch");
  if (int rc = nrx_forward(h, &cio, w.cgnn, w.cgnn_bytes, stream)) return rc;
  return launched(launch_aerial_llr(w.llr, s.batch, s.num_tx, s.num_subcarriers, s.num_symbols, bits_max(&h->desc),
                                    head_bits(&h->desc, 0), io->llr, st),
                  "aerial LLR layout launch");
}

int nrx_llr_demap(const float* llr, int32_t batch, int32_t num_tx, int32_t num_subcarriers, int32_t num_symbols,
                  int32_t bits_stride, int32_t bits, const int32_t* data_re, int32_t n_data, float* out,
                  void* stream) {
  if (!llr || !data_re || !out) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (batch < 1 || num_tx < 1 || num_subcarriers < 1 || num_symbols < 1 || bits < 1 || bits > bits_stride ||
      n_data < 1 || n_data > num_subcarriers * num_symbols)
    return fail(NRX_ERR_SHAPE, "inconsistent demap shape");
  return launched(launch_llr_demap(llr, batch, num_tx, num_subcarriers, num_symbols, bits_stride, bits, data_re,
                                   n_data, out, (hipStream_t)stream),
                  "llr demap launch");
}

static int check_gen(const nrx_gen_desc* d) {
  if (!d) return fail(NRX_ERR_INVALID_ARG, "desc is NULL");
  if (int rc = check_grid_ant(d, kMaxUsers, /*min_subcarriers=*/2)) return rc;
  int mask = 0;
  if (int rc = check_dmrs_symbols(d->dmrs_symbols, d->num_dmrs_symbols, &mask)) return rc;
  if (mask != d->dmrs_symbol_mask) return fail(NRX_ERR_INVALID_ARG, "dmrs_symbol_mask does not match dmrs_symbols");
  if (int rc = check_mcs_bits(d->mcs_bits, d->num_mcs, /*qam=*/true, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_cdm_group(d->cdm_group, d->num_tx)) return rc;
  for (int u = 0; u < d->num_tx; ++u)
    if (d->mcs_of_user[u] < -1 || d->mcs_of_user[u] >= d->num_mcs)
      return fail(NRX_ERR_INVALID_ARG, "mcs_of_user must be -1..num_mcs-1");
  if (d->num_active < 1 || d->num_active > d->num_tx) return fail(NRX_ERR_INVALID_ARG, "num_active must be 1..num_tx");
  if (int rc = check_range("num_taps", d->num_taps, 1, 8, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_range("num_sinusoids", d->num_sinusoids, 1, 16, NRX_ERR_INVALID_ARG)) return rc;
  // an infinite spread or noise power passes, as it always has: only NaN and the sign are refused
  if (!(d->max_delay_s >= 0.0) || !(d->max_doppler_hz >= 0.0) || !(d->subcarrier_spacing > 0.0) || !(d->no >= 0.0))
    return fail(NRX_ERR_INVALID_ARG, "channel parameters must be finite and non-negative (scs > 0)");
  if (d->slot_offset < 0) return fail(NRX_ERR_INVALID_ARG, "slot_offset must be >= 0");
  return NRX_OK;
}

int nrx_gen_workspace_size(const nrx_gen_desc* desc, size_t* bytes) {
  return nrx_gen_workspace_size_cfo(desc, nullptr, bytes);
}

int nrx_generate_slots(const nrx_gen_desc* desc, const nrx_gen_out* out, void* workspace, size_t workspace_bytes,
                       void* stream) {
  return nrx_generate_slots_ex(desc, nullptr, out, workspace, workspace_bytes, stream);
}

// the carrier frequency offset of a generator call: *g resolved for the kernels, *on whether any
// port < U has a non-zero offset (none: the call is nrx_generate_slots_ex)
static int check_gen_cfo(const nrx_gen_desc* d, const nrx_gen_cfo* cfo, GenCfo* g, bool* on) {
  *on = false;
  if (!cfo) return NRX_OK;
  for (int u = 0; u < d->num_tx; ++u) {
    if (int rc = check_nonneg("per-port carrier frequency offset", cfo->cfo_hz[u])) return rc;
    g->eps_max[u] = cfo->cfo_hz[u] / d->subcarrier_spacing;
    *on = *on || cfo->cfo_hz[u] > 0.0;
  }
  if (int rc = check_range("cfo constant", cfo->constant, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_range("h_with_phase", cfo->h_with_phase, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if ((uintptr_t)cfo->eps_out & 7) return fail(NRX_ERR_INVALID_ARG, "eps_out must be 8-byte aligned");
  if (cfo->fft_size)
    if (int rc = check_range("fft_size", cfo->fft_size, d->num_subcarriers, 8192)) return rc;
  g->constant = cfo->constant;
  g->fft_size = cfo->fft_size ? cfo->fft_size : d->num_subcarriers;
  g->h_with_phase = cfo->h_with_phase;
  g->eps_out = cfo->eps_out;
  return NRX_OK;
}

int nrx_gen_workspace_size_cfo(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, size_t* bytes) {
  return nrx_gen_workspace_size_dmrs(desc, cfo, nullptr, bytes);
}

int nrx_generate_slots_ex(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_out* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return nrx_generate_slots_cfo(desc, chan, nullptr, out, workspace, workspace_bytes, stream);
}

int nrx_generate_slots_cfo(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                           const nrx_gen_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  return nrx_generate_slots_dmrs(desc, chan, cfo, nullptr, out, workspace, workspace_bytes, stream);
}

static int check_gen_dmrs(const nrx_gen_desc* d, const nrx_gen_dmrs* dmrs) {
  if (!dmrs) return NRX_OK;
  return check_dmrs_ports(d->num_tx, d->cdm_group, dmrs->focc, dmrs->tocc, dmrs->despread_f, dmrs->despread_t,
                          d->num_subcarriers, d->dmrs_symbols, d->num_dmrs_symbols);
}

int nrx_gen_workspace_size_dmrs(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                                size_t* bytes) {
  return nrx_gen_workspace_size_cir(desc, cfo, dmrs, nullptr, bytes);
}

int nrx_generate_slots_dmrs(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                            const nrx_gen_dmrs* dmrs, const nrx_gen_out* out, void* workspace, size_t workspace_bytes,
                            void* stream) {
  return nrx_generate_slots_cir(desc, chan, cfo, dmrs, nullptr, out, workspace, workspace_bytes, stream);
}

// a replayed channel (nrx_generate_slots_cir), after check_gen
static int check_gen_cir(const nrx_gen_desc* d, const nrx_gen_cir* cir) {
  if (!cir) return NRX_OK;
  if (int rc = check_range("num_examples", cir->num_examples, 1, 1 << 24)) return rc;
  if (int rc = check_range("num_paths", cir->num_paths, 1, 1024)) return rc;
  if (cir->num_time_steps != 1 && cir->num_time_steps != kT)
    return fail(NRX_ERR_SHAPE, "num_time_steps must be 1 or 14");
  if (int rc = check_range("cir select", cir->select, 0, 2, NRX_ERR_INVALID_ARG)) return rc;
  if (cir->select == 2 && cir->num_examples < d->num_tx)
    return fail(NRX_ERR_SHAPE, "select 2 needs num_examples >= num_tx (one example per trajectory)");
  if (!std::isfinite(cir->f_offset)) return fail(NRX_ERR_INVALID_ARG, "f_offset must be finite");
  if (!cir->a || !cir->tau) return fail(NRX_ERR_INVALID_ARG, "null cir dataset pointer");
  if ((uintptr_t)cir->a & 7) return fail(NRX_ERR_INVALID_ARG, "cir a must be 8-byte aligned");
  if (cir->select == 0 && !cir->index) return fail(NRX_ERR_INVALID_ARG, "select 0 needs the cir index");
  return NRX_OK;
}

// The OFDM numerology that nrx_ofdm_io and nrx_gen_td share: N a power of two in 64..4096, F <= N, first_bin
// -1 or 0..N-F, the cyclic prefix of the first T symbols in 0..N; *min_cp (optional): the shortest of them
static int check_ofdm_numerology(int N, const char* f_name, int F, int first_bin, const int32_t* cp, int T,
                                 int* min_cp = nullptr) {
  if (N < 64 || N > 4096 || (N & (N - 1))) return fail(NRX_ERR_SHAPE, "fft_size must be a power of two in 64..4096");
  if (int rc = check_range(f_name, F, 1, N)) return rc;
  if (int rc = check_range("first_bin", first_bin, -1, N - F)) return rc;
  int lo = N;
  for (int t = 0; t < T; ++t) {
    if (int rc = check_range("cp_length", cp[t], 0, N)) return rc;
    lo = cp[t] < lo ? cp[t] : lo;
  }
  if (min_cp) *min_cp = lo;
  return NRX_OK;
}

// the time-domain transmit stage (nrx_generate_slots_td), after check_gen and check_gen_cfo
static int check_gen_td(const nrx_gen_desc* d, const nrx_gen_td* td, bool cfo_on) {
  if (!td) return NRX_OK;
  if (cfo_on) return fail(NRX_ERR_INVALID_ARG, "a td and a cfo with a non-zero offset: one transmit-side stage per call");
  if (int rc = check_ofdm_numerology(td->fft_size, "num_subcarriers", d->num_subcarriers, td->first_bin, td->cp_length, kT)) return rc;
  for (int u = 0; u < d->num_tx; ++u)
    if (td->delay[u] < 0) return fail(NRX_ERR_INVALID_ARG, "per-port delay must be >= 0");
  if (int rc = check_range("pa_enable", td->pa_enable, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_range("h_with_delay", td->h_with_delay, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if (td->pa_enable) {
    if (!std::isfinite(td->pa_ibo_db)) return fail(NRX_ERR_INVALID_ARG, "pa_ibo_db must be finite");
    if (int rc = check_pos("pa_smoothness", td->pa_smoothness)) return rc;
  }
  if ((uintptr_t)td->x_out & 7) return fail(NRX_ERR_INVALID_ARG, "x_out must be 8-byte aligned");
  return NRX_OK;
}

// NULL chan: every port has the desc's scalars, no mixing
static int check_gen_chan(const nrx_gen_desc* desc, const nrx_gen_chan* chan, nrx_gen_chan* c) {
  for (int u = 0; u < desc->num_tx; ++u) {
    c->max_delay_s[u] = chan ? chan->max_delay_s[u] : desc->max_delay_s;
    c->max_doppler_hz[u] = chan ? chan->max_doppler_hz[u] : desc->max_doppler_hz;
    if (!chan) continue;
    if (int rc = check_nonneg("per-port delay spread", c->max_delay_s[u])) return rc;
    if (int rc = check_nonneg("per-port Doppler spread", c->max_doppler_hz[u])) return rc;
  }
  if (chan && ((uintptr_t)chan->rx_mix & 7)) return fail(NRX_ERR_INVALID_ARG, "rx_mix must be 8-byte aligned");
  c->rx_mix = chan ? chan->rx_mix : nullptr;
  return NRX_OK;
}

// the time-domain channel (nrx_generate_slots_tc), after the checks of every other stage; c: the resolved ports
static int check_gen_tc(const nrx_gen_desc* d, const nrx_gen_chan* c, const nrx_gen_tc* tc, bool cfo_on,
                        const nrx_gen_cir* cir, const nrx_gen_td* td) {
  if (!tc) return NRX_OK;
  if (cfo_on) return fail(NRX_ERR_INVALID_ARG, "a tc and a cfo with a non-zero offset: one sample-domain stage per call");
  if (td) return fail(NRX_ERR_INVALID_ARG, "a tc and a td: one sample-domain stage per call");
  if (cir) return fail(NRX_ERR_INVALID_ARG, "a tc and a cir: one sample-domain stage per call");
  int min_cp = 0;
  if (int rc = check_ofdm_numerology(tc->fft_size, "num_subcarriers", d->num_subcarriers, tc->first_bin, tc->cp_length, kT, &min_cp)) return rc;
  if (int rc = check_range("timing_advance", tc->timing_advance, 0, min_cp)) return rc;
  if (int rc = check_tap_span(tc->l_min, tc_resolve_l_max(*d, *c, *tc))) return rc;
  if (((uintptr_t)tc->r_out | (uintptr_t)tc->x_out) & 15) return fail(NRX_ERR_INVALID_ARG, "r_out and x_out must be 16-byte aligned");
  return NRX_OK;
}

// The generator's stage planner: every descriptor check of a generator call in one order, the resolved ports
// (p->c; a NULL chan, as in the size calls that take none: the desc's scalars) and offset (p->cfo, p->cfo_on),
// the stages and the workspace blocks (gen_layout)
static int plan_gen(const nrx_gen_desc* d, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                    const nrx_gen_cir* cir, const nrx_gen_td* td, const nrx_gen_tc* tc, GenPlan* p) {
  if (int rc = check_gen(d)) return rc;
  if (cir && chan) return fail(NRX_ERR_INVALID_ARG, "chan must be NULL with a cir: the dataset is the channel");
  if (int rc = check_gen_chan(d, chan, &p->c)) return rc;
  if (int rc = check_gen_cfo(d, cfo, &p->cfo, &p->cfo_on)) return rc;
  if (int rc = check_gen_dmrs(d, dmrs)) return rc;
  if (int rc = check_gen_cir(d, cir)) return rc;
  if (int rc = check_gen_td(d, td, p->cfo_on)) return rc;
  if (int rc = check_gen_tc(d, &p->c, tc, p->cfo_on, cir, td)) return rc;
  p->d = *d;
  p->dmrs = dmrs, p->cir = cir, p->td = td, p->tc = tc;
  gen_layout(*p);
  return NRX_OK;
}

int nrx_gen_workspace_size_cir(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                               const nrx_gen_cir* cir, size_t* bytes) {
  return nrx_gen_workspace_size_td(desc, cfo, dmrs, cir, nullptr, bytes);
}

int nrx_gen_workspace_size_td(const nrx_gen_desc* desc, const nrx_gen_cfo* cfo, const nrx_gen_dmrs* dmrs,
                              const nrx_gen_cir* cir, const nrx_gen_td* td, size_t* bytes) {
  return nrx_gen_workspace_size_tc(desc, nullptr, cfo, dmrs, cir, td, nullptr, bytes);
}

int nrx_gen_workspace_size_tc(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                              const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                              const nrx_gen_tc* tc, size_t* bytes) {
  GenPlan p{};
  if (int rc = plan_gen(desc, chan, cfo, dmrs, cir, td, tc, &p)) return rc;
  return store_size(bytes, p.total);
}

int nrx_generate_slots_cir(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                           const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_out* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return nrx_generate_slots_td(desc, chan, cfo, dmrs, cir, nullptr, out, workspace, workspace_bytes, stream);
}

int nrx_generate_slots_td(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  return nrx_generate_slots_tc(desc, chan, cfo, dmrs, cir, td, nullptr, out, workspace, workspace_bytes, stream);
}

int nrx_generate_slots_tc(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_tc* tc, const nrx_gen_out* out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return nrx_generate_slots_no(desc, chan, cfo, dmrs, cir, td, tc, nullptr, out, workspace, workspace_bytes, stream);
}

int nrx_generate_slots_no(const nrx_gen_desc* desc, const nrx_gen_chan* chan, const nrx_gen_cfo* cfo,
                          const nrx_gen_dmrs* dmrs, const nrx_gen_cir* cir, const nrx_gen_td* td,
                          const nrx_gen_tc* tc, const nrx_gen_noise* noise, const nrx_gen_out* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
  GenPlan p{};
  if (int rc = plan_gen(desc, chan, cfo, dmrs, cir, td, tc, &p)) return rc;
  p.no_slot = noise ? noise->no_slot : nullptr;
  if ((uintptr_t)p.no_slot & 7) return fail(NRX_ERR_INVALID_ARG, "no_slot must be 8-byte aligned");
  if (!out || !out->y) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (out->bits)
    if (int rc = check_bits_stride(out->bits_stride, desc->mcs_bits, desc->num_mcs)) return rc;
  if ((out->y_real == nullptr) != (out->y_imag == nullptr))
    return fail(NRX_ERR_INVALID_ARG, "Aerial outputs come in (real, imag) pairs");
  if (int rc = check_aerial_list(out->h_ls_real, out->h_ls_imag, desc->num_subcarriers)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, p.total, 1)) return rc;
  return launched(launch_generate(p, *out, workspace, (hipStream_t)stream), "slot generator launch");
}

// nrx_time_channel
static int check_tc(const nrx_tc_io* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->tau || !io->g0 || !io->fd || !io->x || !io->r) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (((uintptr_t)io->g0 | (uintptr_t)io->x | (uintptr_t)io->r | (uintptr_t)io->rx_mix) & 15)
    return fail(NRX_ERR_INVALID_ARG, "g0, x, r and rx_mix must be 16-byte aligned");
  if (((uintptr_t)io->tau | (uintptr_t)io->fd) & 7) return fail(NRX_ERR_INVALID_ARG, "tau and fd must be 8-byte aligned");
  if (int rc = check_pos("sample_rate", io->sample_rate)) return rc;
  if (int rc = check_range("batch", io->batch, 1, 65535)) return rc;
  if (int rc = check_range("num_tx", io->num_tx, 1, kMaxUsers)) return rc;
  if (int rc = check_range("num_rx_ant", io->num_rx_ant, 1, 16)) return rc;
  if (int rc = check_range("num_paths", io->num_paths, 1, 8)) return rc;
  if (int rc = check_range("num_sinusoids", io->num_sinusoids, 1, 16)) return rc;
  if (int rc = check_tap_span(io->l_min, io->l_max)) return rc;
  if (int rc = check_range("num_samples", io->num_samples, 1, 2147483647L)) return rc;
  return check_range("n0", io->n0, -2147483647L - 1, 2147483647L);
}

int nrx_time_channel(const nrx_tc_io* io, void* stream) {
  if (int rc = check_tc(io)) return rc;
  return launched(launch_time_channel(*io, (hipStream_t)stream), "time channel launch");
}

// nrx_ofdm_modulate / nrx_ofdm_demodulate
static int check_ofdm(const nrx_ofdm_io* io, bool modulate) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->grid || !io->samples) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_range("precision", io->precision, NRX_OFDM_F32, NRX_OFDM_F64, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_range("grid_layout", io->grid_layout, NRX_OFDM_GRID_PLANAR, NRX_OFDM_GRID_CGNN,
                           NRX_ERR_INVALID_ARG))
    return rc;
  const uintptr_t real = io->precision == NRX_OFDM_F32 ? 4 : 8;
  if ((uintptr_t)io->samples & (2 * real - 1))
    return fail(NRX_ERR_INVALID_ARG, "samples must be aligned to its complex element");
  if ((uintptr_t)io->grid & ((io->grid_layout == NRX_OFDM_GRID_PLANAR ? 2 * real : real) - 1))
    return fail(NRX_ERR_INVALID_ARG, "grid must be aligned to its element");
  if (modulate && io->pa_asat > 0.0)
    if (int rc = check_pos("pa_smoothness", io->pa_smoothness)) return rc;
  if (int rc = check_range("batch", io->batch, 1, 65535)) return rc;
  if (int rc = check_range("num_streams", io->num_streams, 1, 16)) return rc;
  if (int rc = check_range("num_symbols", io->num_symbols, 1, kT)) return rc;
  int min_cp = 0;
  if (int rc = check_ofdm_numerology(io->fft_size, "grid_subcarriers", io->grid_subcarriers, io->first_bin, io->cp_length,
                                     io->num_symbols, &min_cp))
    return rc;
  if (!modulate)
    if (int rc = check_range("timing_advance", io->timing_advance, 0, min_cp)) return rc;
  const int64_t need = slot_samples(io->cp_length, io->fft_size, io->num_symbols);
  if (io->num_samples < need)
    return fail(NRX_ERR_SHAPE, "num_samples must be >= " + std::to_string(need) + ", the symbols with their prefixes");
  return NRX_OK;
}

int nrx_ofdm_modulate(const nrx_ofdm_io* io, void* stream) {
  if (int rc = check_ofdm(io, true)) return rc;
  return launched(launch_ofdm(*io, true, (hipStream_t)stream), "ofdm modulator launch");
}

int nrx_ofdm_demodulate(const nrx_ofdm_io* io, void* stream) {
  if (int rc = check_ofdm(io, false)) return rc;
  return launched(launch_ofdm(*io, false, (hipStream_t)stream), "ofdm demodulator launch");
}

int nrx_generate_taps(const nrx_gen_desc* desc, const nrx_gen_chan* chan, float* a_out, float* tau_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_gen(desc)) return rc;
  nrx_gen_chan c{};
  if (int rc = check_gen_chan(desc, chan, &c)) return rc;
  if (!a_out || !tau_out) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_workspace(workspace, workspace_bytes, gen_workspace_bytes(*desc, nullptr, nullptr), 1)) return rc;
  return launched(launch_export_taps(*desc, c, a_out, tau_out, workspace, (hipStream_t)stream), "tap export launch");
}

int nrx_ls_estimate(const nrx_ls_io* io, void* stream) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->y || !io->pilots) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (!io->h_hat && !io->h_ls_real && !io->h_ls_imag) return fail(NRX_ERR_INVALID_ARG, "null output pointer");
  if (int rc = check_grid_ant(io)) return rc;
  if (int rc = check_dmrs_symbols(io->dmrs_symbols, io->num_dmrs_symbols)) return rc;
  if (int rc = check_cdm_group(io->cdm_group, io->num_tx)) return rc;
  if (int rc = check_dmrs_ports(io->num_tx, io->cdm_group, io->focc, io->tocc, io->despread_f, io->despread_t,
                                io->num_subcarriers, io->dmrs_symbols, io->num_dmrs_symbols))
    return rc;
  if (int rc = check_aerial_list(io->h_ls_real, io->h_ls_imag, io->num_subcarriers)) return rc;
  return launched(launch_ls_estimate(*io, (hipStream_t)stream), "ls estimator launch");
}

// llr / bits of any slot count, with up to 31 symbols (the mask's bits): not the 14-symbol grid
int nrx_count_errors(const nrx_count_io* io, void* stream) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (!io->llr || !io->bits || !io->active || !io->counts) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (io->batch < 1 || io->num_tx < 1 || io->num_subcarriers < 1 || io->num_symbols < 1 || io->num_symbols > 31 ||
      io->num_heads < 1 || io->num_mcs < 1 || io->num_mcs > 8 || (io->num_heads > 1 && io->num_heads != io->num_mcs))
    return fail(NRX_ERR_SHAPE, "inconsistent counter shape");
  for (int m = 0; m < io->num_mcs; ++m)
    if (io->mcs_bits[m] < 1 || io->mcs_bits[m] > io->bits_stride)
      return fail(NRX_ERR_SHAPE, "mcs_bits must be 1..bits_stride");
  return launched(launch_count_errors(*io, (hipStream_t)stream), "error counter launch");
}

// the fields nrx_lmmse_io and nrx_kbest_io share
extern "C++" {
template <class IO>
static int check_detector(const IO* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->y || !io->h || !io->active || !io->llr) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_pos("no", io->no)) return rc;
  if (int rc = check_nonneg("err_var", io->err_var)) return rc;
  if (int rc = check_mcs_bits(io->mcs_bits, io->num_mcs, /*qam=*/true)) return rc;
  if (int rc = check_grid_ant(io, /*tx_supported=*/8)) return rc;
  return check_bits_stride(io->bits_stride, io->mcs_bits, io->num_mcs);
}
}  // extern "C++"

int nrx_lmmse_detect(const nrx_lmmse_io* io, void* stream) {
  if (int rc = check_detector(io)) return rc;
  return launched(launch_lmmse(*io, (hipStream_t)stream), "lmmse detector launch");
}

static int check_kbest(const nrx_kbest_io* io) {
  if (int rc = check_detector(io)) return rc;
  if (int rc = check_pos("llr_clip", io->llr_clip)) return rc;
  return check_range("k", io->k, 1, 64, NRX_ERR_INVALID_ARG);
}

int nrx_kbest_workspace_size(const nrx_kbest_io* io, size_t* bytes) {
  if (int rc = check_kbest(io)) return rc;
  return store_size(bytes, kbest_workspace_bytes(*io));
}

int nrx_kbest_detect(const nrx_kbest_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_kbest(io)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, kbest_workspace_bytes(*io), 16)) return rc;
  return launched(launch_kbest(*io, workspace, (hipStream_t)stream), "k-best detector launch");
}

// nrx_cov_io and nrx_cov_space_io carry the same fields
extern "C++" {
template <class IO>
static int check_cov(const IO* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->h || !io->acc) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  return check_grid_ant(io);
}
}  // extern "C++"

int nrx_cov_workspace_size(const nrx_cov_io* io, size_t* bytes) {
  if (int rc = check_cov(io)) return rc;
  return store_size(bytes, cov_workspace_bytes(*io));
}

int nrx_cov_accumulate(const nrx_cov_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_cov(io)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, cov_workspace_bytes(*io), 1)) return rc;
  return launched(launch_cov_accumulate(*io, workspace, (hipStream_t)stream), "covariance launch");
}

int nrx_cov_space_workspace_size(const nrx_cov_space_io* io, size_t* bytes) {
  if (int rc = check_cov(io)) return rc;
  return store_size(bytes, cov_space_workspace_bytes(*io));
}

int nrx_cov_space_accumulate(const nrx_cov_space_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_cov(io)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, cov_space_workspace_bytes(*io), 1)) return rc;
  return launched(launch_cov_space(*io, workspace, (hipStream_t)stream), "spatial covariance launch");
}

// the shape, DMRS and group fields that nrx_chest_io and nrx_chest3_io share
extern "C++" {
template <class IO>
static int check_chest_shape(const IO* io) {
  if (int rc = check_grid_ant(io)) return rc;
  if (int rc = check_dmrs_symbols(io->dmrs_symbols, io->num_dmrs_symbols)) return rc;
  return check_cdm_group(io->cdm_group, io->num_tx);
}
}  // extern "C++"

static int check_chest(const nrx_chest_io* io, bool lmmse) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->h_hat || !io->active || !io->h_out) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (lmmse && (!io->filt || !io->tcoef || !io->vconj)) return fail(NRX_ERR_INVALID_ARG, "null table pointer");
  if (lmmse && ((uintptr_t)io->filt & 7)) return fail(NRX_ERR_INVALID_ARG, "filt must be 8-byte aligned");
  if (int rc = check_pos("no", io->no)) return rc;
  return check_chest_shape(io);
}

int nrx_chest_lmmse(const nrx_chest_io* io, void* stream) {
  if (int rc = check_chest(io, true)) return rc;
  return launched(launch_chest_lmmse(*io, (hipStream_t)stream), "lmmse channel estimator launch");
}

int nrx_chest_lin(const nrx_chest_io* io, void* stream) {
  if (int rc = check_chest(io, false)) return rc;
  return launched(launch_chest_lin(*io, (hipStream_t)stream), "linear channel estimator launch");
}

static int check_cfo_io(const nrx_cfo_io* io, bool rotate) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->h_in || !io->eps || !(rotate ? (const void*)io->h_out : (const void*)io->active))
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if ((uintptr_t)io->eps & 7) return fail(NRX_ERR_INVALID_ARG, "eps must be 8-byte aligned");
  if (rotate) {
    if (int rc = check_range("ref_mode", io->ref_mode, NRX_CFO_REF_NEAREST_DMRS, NRX_CFO_REF_ZERO, NRX_ERR_INVALID_ARG))
      return rc;
    if (io->sign != 1 && io->sign != -1) return fail(NRX_ERR_INVALID_ARG, "sign must be +1 or -1");
  }
  return check_chest_shape(io);
}

int nrx_cfo_estimate(const nrx_cfo_io* io, void* stream) {
  if (int rc = check_cfo_io(io, false)) return rc;
  return launched(launch_cfo_estimate(*io, (hipStream_t)stream), "cfo estimator launch");
}

int nrx_cfo_rotate(const nrx_cfo_io* io, void* stream) {
  if (int rc = check_cfo_io(io, true)) return rc;
  return launched(launch_cfo_rotate(*io, (hipStream_t)stream), "cfo rotation launch");
}

static int check_chest3(const nrx_chest3_io* io, bool tables) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (tables) {
    if (!io->h_hat || !io->active || !io->h_out) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
    if (!io->qh || !io->gf || !io->nu || !io->tcoef || !io->vconj || !io->lam || !io->vs || !io->mu)
      return fail(NRX_ERR_INVALID_ARG, "null table pointer");
    if (((uintptr_t)io->qh | (uintptr_t)io->gf) & 7) return fail(NRX_ERR_INVALID_ARG, "qh and gf must be 8-byte aligned");
    if (int rc = check_pos("no", io->no)) return rc;
  }
  return check_chest_shape(io);
}

int nrx_chest3_workspace_size(const nrx_chest3_io* io, size_t* bytes) {
  if (int rc = check_chest3(io, false)) return rc;
  return store_size(bytes, chest3_workspace_bytes(*io));
}

int nrx_chest_lmmse3(const nrx_chest3_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_chest3(io, true)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, chest3_workspace_bytes(*io), 4)) return rc;
  return launched(launch_chest_lmmse3(*io, workspace, (hipStream_t)stream), "3-D lmmse channel estimator launch");
}

// the LLR-tensor fields that nrx_llr_stats_io and nrx_ldpc_gather_io take over from nrx_count_io, on
// the 14-symbol grid and with 1..8 bits per symbol
extern "C++" {
template <class IO>
static int check_llr_grid(const IO* io) {
  if (int rc = check_symbol_mask("dmrs_symbol_mask", io->dmrs_symbol_mask)) return rc;
  if (int rc = check_mcs_bits(io->mcs_bits, io->num_mcs, /*qam=*/false)) return rc;
  if (int rc = check_grid(io)) return rc;
  if (io->num_heads != 1 && io->num_heads != io->num_mcs) return fail(NRX_ERR_SHAPE, "num_heads must be 1 or num_mcs");
  return check_bits_stride(io->bits_stride, io->mcs_bits, io->num_mcs);
}
}  // extern "C++"

static int check_llr_stats(const nrx_llr_stats_io* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->llr || !io->bits || !io->active || !io->loss || !io->cnt || !io->nonfinite)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_range("num_scales", io->num_scales, 1, 16, NRX_ERR_INVALID_ARG)) return rc;
  for (int s = 0; s < io->num_scales; ++s)
    if (int rc = check_pos("scales", io->scales[s])) return rc;
  return check_llr_grid(io);
}

int nrx_llr_stats_workspace_size(const nrx_llr_stats_io* io, size_t* bytes) {
  if (int rc = check_llr_stats(io)) return rc;
  return store_size(bytes, llr_stats_workspace_bytes(*io));
}

int nrx_llr_stats(const nrx_llr_stats_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_llr_stats(io)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, llr_stats_workspace_bytes(*io), 8)) return rc;
  return launched(launch_llr_stats(*io, workspace, (hipStream_t)stream), "llr statistics launch");
}

static int check_nmse(const nrx_nmse_io* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->h_est || !io->h_true || !io->active || !io->err || !io->ref || !io->items)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_symbol_mask("symbol_mask", io->symbol_mask)) return rc;
  return check_grid_ant(io);
}

int nrx_nmse_workspace_size(const nrx_nmse_io* io, size_t* bytes) {
  if (int rc = check_nmse(io)) return rc;
  return store_size(bytes, nmse_workspace_bytes(*io));
}

int nrx_chest_nmse(const nrx_nmse_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_nmse(io)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, nmse_workspace_bytes(*io), 8)) return rc;
  return launched(launch_chest_nmse(*io, workspace, (hipStream_t)stream), "channel nmse launch");
}

// ---- QC-LDPC decoder: the host table is validated and packed into per-layer edge lists
struct nrx_ldpc {
  LdpcDev d;
  int device;                  // -1: no device tables (sizing and argument checks only)
  void* tables;                // one device allocation: row_ptr, then edges
};

constexpr int kLdpcMaxN = 68 * 384;

int nrx_ldpc_create(const nrx_ldpc_code* code, int32_t device, nrx_ldpc** out) {
  if (!code || !code->shifts || !out) return fail(NRX_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int mb = code->mb, nb = code->nb, z = code->z;
  if (mb < 1 || mb > 46) return fail(NRX_ERR_SHAPE, "mb must be 1..46");
  if (nb < 2 || nb > 68) return fail(NRX_ERR_SHAPE, "nb must be 2..68");
  if (nb <= mb) return fail(NRX_ERR_SHAPE, "nb must be > mb");
  if (z < 2 || z > 384) return fail(NRX_ERR_SHAPE, "z must be 2..384");
  if (code->kb < 1 || code->kb >= nb) return fail(NRX_ERR_SHAPE, "kb must be 1..nb-1");
  if (device < -1) return fail(NRX_ERR_INVALID_ARG, "device must be >= 0, or -1 for a handle without device tables");
  std::vector<int> row_ptr(mb + 1, 0), edges, colw(nb, 0);
  for (int i = 0; i < mb; ++i) {
    for (int j = 0; j < nb; ++j) {
      const int s = code->shifts[i * nb + j];
      if (s < -1 || s >= z) return fail(NRX_ERR_INVALID_ARG, "shifts must be -1..z-1");
      if (s < 0) continue;
      edges.push_back(j * z);
      edges.push_back(s);
      colw[j] += 1;
    }
    row_ptr[i + 1] = (int)edges.size() / 2;
    const int w = row_ptr[i + 1] - row_ptr[i];
    if (w < 2 || w > 32) return fail(NRX_ERR_INVALID_ARG, "row weight must be 2..32");
  }
  for (int j = 0; j < nb; ++j)
    if (!colw[j]) return fail(NRX_ERR_INVALID_ARG, "column weight must be >= 1");
  nrx_ldpc* h = new nrx_ldpc();
  h->d.mb = mb, h->d.nb = nb, h->d.z = z, h->d.kb = code->kb, h->d.num_edges = row_ptr[mb];
  h->d.plan = ldpc_plan(nb, z, h->d.num_edges);
  h->d.row_ptr = nullptr, h->d.edges = nullptr;
  h->device = device;
  h->tables = nullptr;
  if (device >= 0) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = ldpc_setup();
    const size_t rp = (size_t)(mb + 1) * 4, rpa = (rp + 15) / 16 * 16, eb = edges.size() * 4;
    if (e == hipSuccess) e = hipMalloc(&h->tables, rpa + eb);
    if (e == hipSuccess) e = hipMemcpy(h->tables, row_ptr.data(), rp, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)h->tables + rpa, edges.data(), eb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (h->tables) (void)hipFree(h->tables);
      delete h;
      return hip_fail(e, "ldpc tables");
    }
    h->d.row_ptr = (const int*)h->tables;
    h->d.edges = (const int*)((char*)h->tables + rpa);
  }
  *out = h;
  return NRX_OK;
}

void nrx_ldpc_destroy(nrx_ldpc* h) {
  if (!h) return;
  if (h->tables) (void)hipFree(h->tables);
  delete h;
}

static int check_ldpc_io(const nrx_ldpc_io* io) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->llr_in || !io->hard || !io->iters || !io->parity_ok) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_range("num_iter", io->num_iter, 1, 100, NRX_ERR_INVALID_ARG)) return rc;
  if (io->cn_type != 0 && io->cn_type != 1) return fail(NRX_ERR_INVALID_ARG, "cn_type must be 0 (boxplus) or 1 (min-sum)");
  if (io->early_stop != 0 && io->early_stop != 1) return fail(NRX_ERR_INVALID_ARG, "early_stop must be 0 or 1");
  if (io->cn_type == 1 && !(io->ms_scale > 0.0f && io->ms_scale <= 1.0f))
    return fail(NRX_ERR_INVALID_ARG, "ms_scale must be in (0, 1]");
  if (int rc = check_pos("llr_clip", io->llr_clip)) return rc;
  return check_range("num_cw", io->num_cw, 1, 1 << 20);
}

static size_t ldpc_workspace_bytes(const nrx_ldpc* h, const nrx_ldpc_io* io) {
  const size_t msgs = h->d.plan.msg_lds ? 0 : (size_t)io->num_cw * h->d.num_edges * h->d.z * 4;
  return msgs > 256 ? msgs : 256;
}

int nrx_ldpc_workspace_size(const nrx_ldpc* h, const nrx_ldpc_io* io, size_t* bytes) {
  if (int rc = check_ldpc_io(io)) return rc;
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null handle");
  return store_size(bytes, ldpc_workspace_bytes(h, io));
}

int nrx_ldpc_decode(nrx_ldpc* h, const nrx_ldpc_io* io, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_ldpc_io(io)) return rc;
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null handle");
  if (int rc = check_workspace(workspace, workspace_bytes, ldpc_workspace_bytes(h, io), 16)) return rc;
  if (h->device < 0) return fail(NRX_ERR_INVALID_ARG, "no device: the handle was created with device = -1");
  return launched(launch_ldpc_decode(h->d, *io, workspace, (hipStream_t)stream), "ldpc decode launch");
}

int nrx_ldpc_gather(const nrx_ldpc_gather_io* io, void* stream) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->llr || !io->bits || !io->active || !io->llr_in || !io->skip)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_llr_grid(io)) return rc;
  if (int rc = check_range("num_cw_per_user", io->num_cw_per_user, 1, 64)) return rc;
  if (int rc = check_range("n", io->n, 4, kLdpcMaxN)) return rc;
  if ((int64_t)io->batch * io->num_tx * io->num_cw_per_user > (1 << 20))
    return fail(NRX_ERR_SHAPE, "batch * num_tx * num_cw_per_user must be <= 2^20");
  if (int rc = check_range("n_tx", io->n_tx, 1, 1 << 20)) return rc;
  if (!io->tx_col && io->n_tx > io->n) return fail(NRX_ERR_SHAPE, "n_tx > n needs a tx_col");
  return launched(launch_ldpc_gather(*io, (hipStream_t)stream), "ldpc gather launch");
}

int nrx_ldpc_count(const nrx_ldpc_count_io* io, void* stream) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->hard || !io->skip || !io->counts) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (int rc = check_range("batch", io->batch, 1, 65535)) return rc;
  if (int rc = check_range("num_tx", io->num_tx, 1, kMaxUsers)) return rc;
  if (int rc = check_range("num_cw_per_user", io->num_cw_per_user, 1, 64)) return rc;
  if (int rc = check_range("n", io->n, 4, kLdpcMaxN)) return rc;
  if (io->num_info < 1 || io->num_info > io->n) return fail(NRX_ERR_SHAPE, "num_info must be 1..n");
  return launched(launch_ldpc_count(*io, (hipStream_t)stream), "ldpc count launch");
}

// ---- training: the topology check is nrx_create's, the grid check nrx_forward's
static int check_aligned(const char* name, const void* p, size_t align) {
  if (!((uintptr_t)p & (align - 1))) return NRX_OK;
  return fail(NRX_ERR_INVALID_ARG, std::string(name) + " must be " + std::to_string(align) + "-byte aligned");
}

static int check_train(const nrx_desc* d, const nrx_train_io* io) {
  if (int rc = check_desc(d)) return rc;
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (int rc = check_shape(&io->shape)) return rc;
  if ((int64_t)io->shape.batch * io->shape.num_tx * io->shape.num_subcarriers * kT > (1 << 24))
    return fail(NRX_ERR_SHAPE, "training takes at most 2^24 positions (batch x num_tx x num_subcarriers x 14)");
  if (io->num_it < 1 || io->num_it > d->num_it) return fail(NRX_ERR_INVALID_ARG, "Invalid number of iterations");
  if (int rc = check_symbol_mask("dmrs_symbol_mask", io->dmrs_symbol_mask)) return rc;
  if (io->dmrs_symbol_mask == (1 << kT) - 1)
    return fail(NRX_ERR_INVALID_ARG, "dmrs_symbol_mask must leave a data symbol");
  if (int rc = check_range("multiloss", io->multiloss, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
  if (int rc = check_nonneg("w_chest", io->w_chest)) return rc;
  if (int rc = check_bits_stride(io->bits_stride, d->bits, d->num_mcs)) return rc;
  if (!io->y || !io->pe || !io->active || !io->bits || !io->weights || !io->grad || !io->loss)
    return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  if (d->use_h_hat && !io->h_hat) return fail(NRX_ERR_INVALID_ARG, "h_hat is required by this model");
  if (io->w_chest > 0.0 && !io->h) return fail(NRX_ERR_INVALID_ARG, "h is required when w_chest > 0");
  const void* f32s[] = {io->y, io->pe, io->h_hat, io->active, io->mcs_mask, io->h, io->weights, io->grad, io->llr,
                        io->h_ref};
  for (const void* p : f32s)
    if (int rc = check_aligned("float tensors", p, 4)) return rc;
  return check_aligned("loss", io->loss, 8);
}

int nrx_train_workspace_size(const nrx_desc* desc, const nrx_train_io* io, size_t* bytes) {
  if (int rc = check_train(desc, io)) return rc;
  return store_size(bytes, train_workspace_bytes(*desc, *io));
}

int nrx_train_grad(const nrx_desc* desc, const nrx_train_io* io, void* workspace, size_t workspace_bytes,
                   void* stream) {
  return nrx_train_grad_acc(desc, io, nullptr, workspace, workspace_bytes, stream);
}

int nrx_train_grad_acc(const nrx_desc* desc, const nrx_train_io* io, const nrx_train_acc* acc, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (int rc = check_train(desc, io)) return rc;
  if (acc) {
    if (int rc = check_range("accumulate", acc->accumulate, 0, 1, NRX_ERR_INVALID_ARG)) return rc;
    if (acc->batch_total < io->shape.batch || acc->batch_total > 65535)
      return fail(NRX_ERR_SHAPE, "batch_total must be shape.batch..65535");
  }
  if (int rc = check_workspace(workspace, workspace_bytes, train_workspace_bytes(*desc, *io), 256)) return rc;
  return launched(launch_train_grad(*desc, *io, acc && acc->accumulate, acc ? acc->batch_total : io->shape.batch,
                                    workspace, (hipStream_t)stream),
                  "training launch");
}

int nrx_adam_step(const nrx_adam_io* io, void* stream) {
  if (!io) return fail(NRX_ERR_INVALID_ARG, "io is NULL");
  if (!io->w || !io->g || !io->m || !io->v) return fail(NRX_ERR_INVALID_ARG, "null tensor pointer");
  const void* f32s[] = {io->w, io->g, io->m, io->v};
  for (const void* p : f32s)
    if (int rc = check_aligned("float tensors", p, 4)) return rc;
  if (io->n < 0) return fail(NRX_ERR_INVALID_ARG, "n must be >= 0");
  if (io->step < 1) return fail(NRX_ERR_INVALID_ARG, "step must be >= 1");
  if (int rc = check_nonneg("lr", io->lr)) return rc;
  if (int rc = check_nonneg("eps", io->eps)) return rc;
  if (!(io->beta1 >= 0.0 && io->beta1 < 1.0) || !(io->beta2 >= 0.0 && io->beta2 < 1.0))
    return fail(NRX_ERR_INVALID_ARG, "beta1 and beta2 must be in [0, 1)");
  const double c1 = 1.0 - std::pow(io->beta1, (double)io->step), c2 = 1.0 - std::pow(io->beta2, (double)io->step);
  return launched(launch_adam(*io, c1, c2, (hipStream_t)stream), "adam launch");
}

int nrx_profile_enable(nrx_handle* h, int32_t enable) {
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null handle");
  if (enable) {
    if (!h->prof) h->prof = new EventProf();
    hipError_t e = h->prof->collect();
    h->prof->reset();
    if (e != hipSuccess) return hip_fail(e, "profile reset");
  } else {
    delete h->prof;
    h->prof = nullptr;
  }
  return NRX_OK;
}

int nrx_fused_status(nrx_handle* h, int32_t* status, int32_t reset) {
  if (!h || !status) return fail(NRX_ERR_INVALID_ARG, "null argument");
  int st[3] = {0, 0, 0};
  hipError_t e = fused_sync_status(h->fused_sync, st, reset != 0, h->have_last ? h->last_ev : nullptr);
  if (e != hipSuccess) return hip_fail(e, "fused status");
  for (int i = 0; i < 3; ++i) status[i] = st[i];
  if (st[0])
    return fail(NRX_ERR_FUSED, "one-launch forward error bits " + std::to_string(st[0]) +
                                   " (1: dependency wait timed out, 2: items left undone): outputs invalid");
  return NRX_OK;
}

int nrx_fused_config(nrx_handle* h, int32_t enable, int32_t spin_limit, int32_t inject_err) {
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null argument");
  // every argument < 0 leaves its setting unchanged; spin_limit == 0 restores the
  // default bound
  if (enable > 2) return fail(NRX_ERR_INVALID_ARG, "enable must be 0 (off), 1 (default) or 2 (force)");
  if (enable >= 0) h->fused_enabled = enable;
  if (spin_limit >= 0) h->spin_limit = spin_limit > 0 ? spin_limit : kFusedSpinLimit;
  if (inject_err >= 0) h->dbg_err = inject_err;
  return NRX_OK;
}

int nrx_update_schedule(nrx_handle* h, int32_t update_rr) {
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (update_rr > kSchedMax) return fail(NRX_ERR_INVALID_ARG, "update_rr is a stage mask 0..127");
  if (update_rr >= 0) h->update_rr = update_rr;
  return NRX_OK;
}

// Tests only (not in include/nrx.h): the small-grid strip tiers (8 / 16-row strips) off or on for this handle, so that
// a test can run the 24-row tier's kernels -- the column launches among them -- on a handful of slots.  enable < 0
// leaves the setting.  Every tier computes the same bits.
int nrx_debug_small_tiers(nrx_handle* h, int32_t enable) {
  if (!h) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (enable >= 0) h->small_tiers = enable != 0;
  return NRX_OK;
}

// The launch plan of a forward, without a handle (tests only, like nrx_probe_buffer_oob: not in include/nrx.h): the
// checks, the chunking and the plan_forward of nrx_forward, at cus / xccs (cus == 0: the current device's; else no
// HIP call).  Into out[cap], 16 int32 per chunk (b0, n, -1, FwdPlan's 11 fields up to nq, one_launch, combine launches)
// and per stage s (b0, n, s, StagePlan's 11 fields up to order_rev, its variant, 0).  Returns the int32 count of the whole plan or an error code.
// nrx_debug_forward_plan_io: the same for a caller that hands the optional tensors named by io_flags (1: h_ref, 2: an
// MCS mask), which the plan of the column launches looks at (StagePlan::variant).
static int debug_forward_plan(const nrx_desc* desc, const nrx_shape* shape, int32_t precision, int32_t num_it,
                              int32_t sched_mask, int32_t fused_mode, int32_t cus, int32_t xccs, int32_t io_flags,
                              int32_t* out, int32_t cap) {
  if (int rc = check_desc(desc)) return rc;
  if (int rc = check_shape(shape)) return rc;
  if (precision != NRX_PREC_F16 && precision != NRX_PREC_F32X) return fail(NRX_ERR_INVALID_ARG, "unknown precision");
  if (num_it < 1 || num_it > desc->num_it) return fail(NRX_ERR_INVALID_ARG, "Invalid number of iterations");
  if (sched_mask < 0 || sched_mask > kSchedMax || fused_mode < 0 || fused_mode > 2 || cus < 0 || (!out && cap > 0))
    return fail(NRX_ERR_INVALID_ARG, "bad schedule, device counts or output");
  if (cus == 0) device_counts(&cus, &xccs);
  nrx_io io{*shape, num_it, precision};
  void* ws = reinterpret_cast<void*>(uintptr_t(256));   // a dummy base: pe16 non-null, nothing is dereferenced
  if (io_flags & 1) io.h_ref = reinterpret_cast<float*>(ws);
  if (io_flags & 2) io.mcs_mask = reinterpret_cast<const float*>(ws);
  int n_out = 0;
  auto put = [&](int b0, int n, int s, const void* plan, int x, int y) {
    int rec[16] = {b0, n, s};
    memcpy(rec + 3, plan, 11 * sizeof(int));   // the leading int fields of a FwdPlan / all of a StagePlan
    rec[14] = x, rec[15] = y;
    for (int k = 0; k < 16; ++k, ++n_out)
      if (n_out < cap) out[n_out] = rec[k];
  };
  static_assert(offsetof(FwdPlan, st) == 11 * sizeof(int) && offsetof(StagePlan, variant) == 11 * sizeof(int) &&
                    sizeof(StagePlan) == 12 * sizeof(int),
                "record layout");
  (void)each_chunk(shape, precision, [&](int b0, int n) {
    FwdPlan pl;
    if (precision == NRX_PREC_F16) {
      FwdArgs<_Float16, float, _Float16> a{};
      pl = plan_f16(a, desc, &io, n, ws, init_padded_cin(desc, 32), Sched{sched_mask, fused_mode}, cus, xccs);
    } else {
      FwdArgs<double, double, float> a{};
      nrx_io c = io;
      c.shape.batch = n;
      fill_args(a, desc, &c, ws, init_padded_cin(desc, 16));
      pl = plan_forward(a, num_it);
    }
    put(b0, n, -1, &pl, pl.one_launch(), pl.combine_launches());
    for (int s = 0; s < pl.num_init + pl.num_it; ++s) put(b0, n, s, &pl.st[s], pl.st[s].variant, 0);
    return 0;
  });
  return n_out;
}

int nrx_debug_forward_plan(const nrx_desc* desc, const nrx_shape* shape, int32_t precision, int32_t num_it,
                           int32_t sched_mask, int32_t fused_mode, int32_t cus, int32_t xccs, int32_t* out,
                           int32_t cap) {
  return debug_forward_plan(desc, shape, precision, num_it, sched_mask, fused_mode, cus, xccs, 0, out, cap);
}

int nrx_debug_forward_plan_io(const nrx_desc* desc, const nrx_shape* shape, int32_t precision, int32_t num_it,
                              int32_t sched_mask, int32_t fused_mode, int32_t cus, int32_t xccs, int32_t io_flags,
                              int32_t* out, int32_t cap) {
  if (io_flags < 0 || io_flags > 3) return fail(NRX_ERR_INVALID_ARG, "io_flags: 1 h_ref, 2 mcs_mask");
  return debug_forward_plan(desc, shape, precision, num_it, sched_mask, fused_mode, cus, xccs, io_flags, out, cap);
}

int nrx_profile_read(nrx_handle* h, int32_t kernel, int64_t* launches, double* total_ms) {
  if (!h || !launches || !total_ms) return fail(NRX_ERR_INVALID_ARG, "null argument");
  if (kernel < 0 || kernel >= K_COUNT) return fail(NRX_ERR_INVALID_ARG, "bad kernel id");
  if (!h->prof) return fail(NRX_ERR_INVALID_ARG, "profiling is not enabled");
  hipError_t e = h->prof->collect();
  if (e != hipSuccess) return hip_fail(e, "profile collect");
  *launches = h->prof->launches[kernel];
  *total_ms = h->prof->total_ms[kernel];
  return NRX_OK;
}

// Product-side restatement of the nearest-pilot positional encoding
// (onnx_utils.py:206-260).  Pilots of CDM group g (DMRS config type 1)
// occupy subcarriers f with f % 2 == g on the DMRS symbols.
int nrx_compute_pe(int32_t num_tx, int32_t F, int32_t T, const int32_t* dmrs_symbols, int32_t nsym,
                   const int32_t* cdm_group, float* pe) {
  if (num_tx < 1 || F < 1 || T < 1 || !dmrs_symbols || nsym < 1 || !cdm_group || !pe)
    return fail(NRX_ERR_INVALID_ARG, "bad argument");
  std::vector<double> dt(T), df(F);
  for (int u = 0; u < num_tx; ++u) {
    if (cdm_group[u] != 0 && cdm_group[u] != 1) return fail(NRX_ERR_INVALID_ARG, "cdm_group must be 0/1");
    bool any_f = false;
    for (int t = 0; t < T; ++t) {
      int best = 1 << 30;
      for (int k = 0; k < nsym; ++k) best = std::min(best, std::abs(dmrs_symbols[k] - t));
      dt[t] = best;
    }
    for (int f = 0; f < F; ++f) {
      int best = 1 << 30;
      for (int p = cdm_group[u]; p < F; p += 2) {
        best = std::min(best, std::abs(p - f));
        any_f = true;
      }
      df[f] = best;
    }
    if (!any_f) return fail(NRX_ERR_INVALID_ARG, "user has no pilots");
    // normalise: time over the symbol axis, frequency over the subcarrier axis;
    // population std, left unscaled where std == 0
    auto norm = [](std::vector<double>& v) {
      double m = 0;
      for (double x : v) m += x;
      m /= v.size();
      double s2 = 0;
      for (double& x : v) {
        x -= m;
        s2 += x * x;
      }
      const double sd = std::sqrt(s2 / v.size());
      if (sd > 0)
        for (double& x : v) x /= sd;
    };
    norm(dt);
    norm(df);
    for (int f = 0; f < F; ++f)
      for (int t = 0; t < T; ++t) {
        pe[(((size_t)u * F + f) * T + t) * 2 + 0] = (float)dt[t];
        pe[(((size_t)u * F + f) * T + t) * 2 + 1] = (float)df[f];
      }
  }
  return NRX_OK;
}

double nrx_flops_per_re_user(const nrx_desc* d, int32_t num_it) {
  return check_desc(d) ? 0.0 : flops_per_re_user(d, num_it);
}

}  // extern "C"
