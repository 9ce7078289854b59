// Host runtime + C-ABI of libdebvader_hip.so (see include/debvader_hip.h).
//
// Replaces, for the hot path only, what Keras/TFP do under debvader's Python surface:
//   create_model_vae            src/debvader/model/model.py:164-218   -> dv_model_create / dv_model_init
//   net.fit train/test function src/debvader/training/train.py:27-37  -> dv_train_step / dv_eval_step
//   net.compile(legacy Adam)    src/debvader/training/train.py:125-130,178-183 -> dv_optimizer_reset
//   net(x) inside deblend()     src/debvader/deblend_cutout/deblender.py:18    -> dv_infer
// One process drives one GPU; ranks are joined with RCCL (gradient / BN-statistic / loss all-reduce).
// All activations are NHWC fp32 in HBM, weights + Adam slots live in three flat buffers with the
// same layout so that one all-reduce and one fused Adam launch cover every trainable tensor.
#include <rccl/rccl.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <set>
#include <vector>
#ifdef DV_DEBUG_EXPORTS
#include <functional>
#endif

#include "../../include/debvader_hip.h"
#ifdef DV_DEBUG_EXPORTS
#include "../../include/debvader_hip_debug.h"
#endif
#include <chrono>
#include "common.h"
#include "rows.h"
#include "bf16.h"

namespace dv {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) at %s:%d in %s", (int)e, hipGetErrorString(e), file, line, what);
  return e == hipErrorOutOfMemory ? E_NOMEM : E_HIP;
}
#define DV_NCCL(call)                                                                      \
  do {                                                                                     \
    ncclResult_t r__ = (call);                                                             \
    if (r__ != ncclSuccess) {                                                              \
      dv::set_error("RCCL error %d (%s) in %s", (int)r__, ncclGetErrorString(r__), #call); \
      return dv::E_RCCL;                                                                   \
    }                                                                                      \
  } while (0)

// --------------------------------------------------------------------------------------------
// architecture plan
// --------------------------------------------------------------------------------------------
struct Spec {
  std::string name;
  int64_t shape[4];
  int ndim;
  bool trainable;
  size_t count;
  size_t off;  // offset in the flat parameter buffer (floats)
};

// DV_EXP_SKIP_TAIL=<bits> (MEASUREMENT switch, wrong results): what the serial seams of a train step cost.  1: the tail of
// the shallow gradient bucket (slab / partial sums behind the last weight gradient, first-conv gradients, Adam of the last
// range, BN fold, bf16 cast / Winograd transform).  2: the loss sums and the head's bias column sums on the main stream
// between the forward and the backward pass.  4 (fp32): bn_finalize + bn_apply at the head of the step.
static int exp_skip_tail() {
  static const int v = DV_EXP_SWITCH("DV_EXP_SKIP_TAIL");
  return v;
}

// DV_EXP_SKIP_SMALL=1 (a MEASUREMENT switch, results are wrong): the elementwise neighbours of the dense trunk that a fused
// trunk would absorb (split-K finish, the two PReLU forwards, the narrow dense data gradient, the bias column sums, the
// bf16 seam conversions) are not launched - the upper bound of what merging them can give the step
#ifdef DV_DEBUG_EXPORTS
int exp_switch(const char* name) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  if (v != 0) {
    static std::mutex mu;
    static std::set<std::string> told;
    std::lock_guard<std::mutex> g(mu);
    if (told.insert(name).second)
      fprintf(stderr, "[libdebvader_hip_debug] WARNING: %s=%d is a MEASUREMENT switch - work is left out, every result of "
                      "this process is WRONG\n", name, v);
  }
  return v;
}
#endif
static bool exp_skip_small() {
  static const bool v = DV_EXP_SWITCH("DV_EXP_SKIP_SMALL") >= 1;
  return v;
}
// DV_EXP_SKIP_SMALL=2: additionally none of the dense trunk's matrix launches (forward, data gradient, weight gradient)
static bool exp_skip_dense() {
  static const bool v = DV_EXP_SWITCH("DV_EXP_SKIP_SMALL") >= 2;
  return v;
}

static int same_pad_before(int n_in, int k, int s, int* n_out) {
  int o = (n_in + s - 1) / s;
  int tot = std::max((o - 1) * s + k - n_in, 0);
  if (n_out) *n_out = o;
  return tot / 2;
}

struct Arch {
  dv_config cfg;
  int H = 0, C = 0, d = 0, L = 0;
  int tw = 0, dec_hidden = 0, w0 = 0, flat = 0, dec_out = 0, crop0 = 0;
  // row strides of the latent-sized tensors (t, d(t): twp; eps, z, stddev, the decoder's input: dp): tw and d padded to
  // multiples of 4 floats for the 16-byte accesses of the dense kernels; the pad columns carry zeros
  int twp = 0, dp = 0;
  int C2p = 0;  // head output channels as stored: 2*bands padded to a multiple of 16
  int C0p = 8;  // channels of the normalised input as stored: bands + the constant 1 that carries the BatchNorm shift, padded to 8 or 16
  std::vector<int> enc_sizes;
  std::vector<Spec> specs;
  size_t n_enc_train = 0, n_train = 0, n_total = 0;  // flat counts incl. alignment padding
  int64_t n_enc_params = 0, n_dec_params = 0, n_trainable_params = 0;
  int D0 = 0;

  // kernel size of encoder conv j / decoder conv-transpose j (model.py:81-91: both convs of level i use kernels[i];
  // model.py:120-134: the decoder walks the levels in reverse)
  int enc_ksz(int j) const { return cfg.kernels[j / 2]; }
  int dec_ksz(int j) const { return cfg.kernels[L - 1 - j / 2]; }
  int enc_k(int j) const { return 4 + 3 * j; }
  int enc_b(int j) const { return 5 + 3 * j; }
  int enc_al(int j) const { return 6 + 3 * j; }
  int enc_flat_al() const { return 4 + 6 * L; }
  int enc_dk() const { return 5 + 6 * L; }
  int enc_db() const { return 6 + 6 * L; }
  int dec_k(int j) const { return D0 + 7 + 3 * j; }
  int dec_b(int j) const { return D0 + 8 + 3 * j; }
  int dec_al(int j) const { return D0 + 9 + 3 * j; }
  int head_k() const { return D0 + 7 + 6 * L; }
  int head_b() const { return D0 + 8 + 6 * L; }

  // encoder conv j: input size/channels, output size/channels, stride
  void enc_layer(int j, int* hin, int* cin, int* hout, int* cout, int* s) const {
    int lvl = j / 2;
    *s = (j % 2) ? 2 : 1;
    *hin = enc_sizes[lvl];
    *hout = (j % 2) ? enc_sizes[lvl + 1] : enc_sizes[lvl];
    *cout = cfg.filters[lvl];
    *cin = (j % 2) ? cfg.filters[lvl] : (lvl == 0 ? C : cfg.filters[lvl - 1]);
  }
  // decoder convT j (reference iterates filters in reverse, model.py:120)
  void dec_layer(int j, int* hin, int* cin, int* hout, int* cout, int* s) const {
    int jj = j / 2;
    int lvl = L - 1 - jj;
    *s = (j % 2) ? 1 : 2;
    int size_in = w0 << jj;
    *hin = (j % 2) ? size_in * 2 : size_in;
    *hout = size_in * 2;
    *cout = cfg.filters[lvl];
    *cin = (j % 2) ? cfg.filters[lvl] : (jj == 0 ? cfg.filters[L - 1] : cfg.filters[lvl + 1]);
  }

  int build(const dv_config* c) {
    cfg = *c;
    H = c->height;
    C = c->bands;
    d = c->latent_dim;
    L = c->n_levels;
    if (c->height != c->width) {
      set_error("only square stamps are supported (reference uses input_shape[0] for both axes)");
      return E_INVALID;
    }
    if (L < 1 || L > DV_MAX_LEVELS || C < 1 || C > 15 || d < 1 || H < 4) {
      set_error("unsupported architecture (levels=%d bands=%d latent=%d size=%d)", L, C, d, H);
      return E_INVALID;
    }
    for (int i = 0; i < L; ++i) {
      if (c->kernels[i] < 1 || c->kernels[i] > 5) {
        set_error("kernel sizes 1 .. 5 are implemented (kernels[%d]=%d)", i, c->kernels[i]);
        return E_INVALID;
      }
      if (c->filters[i] < 4 || (c->filters[i] & 3)) {
        set_error("filters must be multiples of 4");
        return E_INVALID;
      }
    }
    // any latent_dim (d > 64: the workgroup-per-stamp sampler kernels); what bounds it is the 32-bit element offsets
    // of the kernels that address one parameter tensor, the largest of which is the encoder Dense kernel [flat][tw]
    const int64_t tw64 = (int64_t)d + (int64_t)d * (d + 1) / 2;
    const int64_t flat64 = (int64_t)((H + (1 << L) - 1) >> L) * ((H + (1 << L) - 1) >> L) * c->filters[L - 1];
    // (its padded copies: [flat][twp] fp32, [tw padded to 64][flat] bf16)
    if (flat64 * ((tw64 + 63) & ~(int64_t)63) >= ((int64_t)1 << 31)) {
      set_error("latent_dim %d: the encoder Dense kernel (%lld x %lld, padded) reaches 2^31 elements; a parameter tensor "
                "must stay below 2^31 elements (32-bit element offsets)", d, (long long)flat64, (long long)tw64);
      return E_INVALID;
    }
    tw = d + d * (d + 1) / 2;
    twp = (tw + 3) & ~3;
    dp = (d + 3) & ~3;
    dec_hidden = 32 + 32 * 33 / 2;  // hard-coded params_size(32), model.py:114
    enc_sizes.assign(1, H);
    for (int i = 0; i < L; ++i) enc_sizes.push_back((enc_sizes.back() + 1) / 2);
    w0 = (H + (1 << L) - 1) >> L;  // ceil(H / 2^L), model.py:116
    flat = enc_sizes[L] * enc_sizes[L] * c->filters[L - 1];
    dec_out = w0 << L;
    int crop = dec_out - H;
    crop0 = crop > 0 ? crop / 2 : 0;  // model.py:140-148
    if (crop < 0) {
      set_error("decoder output smaller than the stamp");
      return E_INVALID;
    }
    D0 = 7 + 6 * L;
    C2p = ((2 * C + 15) / 16) * 16;
    C0p = C < 8 ? 8 : 16;
    specs.clear();
    auto add = [&](const std::string& n, std::vector<int64_t> sh, bool tr) {
      Spec s;
      s.name = n;
      s.ndim = (int)sh.size();
      s.count = 1;
      for (int i = 0; i < 4; ++i) s.shape[i] = i < s.ndim ? sh[i] : 1;
      for (int i = 0; i < s.ndim; ++i) s.count *= (size_t)sh[i];
      s.trainable = tr;
      s.off = 0;
      specs.push_back(s);
    };
    add("enc/bn/gamma", {C}, true);
    add("enc/bn/beta", {C}, true);
    add("enc/bn/moving_mean", {C}, false);
    add("enc/bn/moving_variance", {C}, false);
    for (int j = 0; j < 2 * L; ++j) {
      int hin, cin, hout, cout, s;
      enc_layer(j, &hin, &cin, &hout, &cout, &s);
      char b[64];
      snprintf(b, sizeof b, "enc/conv%d/kernel", j);
      add(b, {enc_ksz(j), enc_ksz(j), cin, cout}, true);
      snprintf(b, sizeof b, "enc/conv%d/bias", j);
      add(b, {cout}, true);
      snprintf(b, sizeof b, "enc/prelu%d/alpha", j);
      add(b, {hout, hout, cout}, true);
    }
    add("enc/prelu_flat/alpha", {flat}, true);
    add("enc/dense/kernel", {flat, tw}, true);
    add("enc/dense/bias", {tw}, true);
    int r = w0 * w0 * c->filters[L - 1];
    add("dec/prelu_in/alpha", {d}, true);
    add("dec/dense0/kernel", {d, dec_hidden}, true);
    add("dec/dense0/bias", {dec_hidden}, true);
    add("dec/prelu_h/alpha", {dec_hidden}, true);
    add("dec/dense1/kernel", {dec_hidden, r}, true);
    add("dec/dense1/bias", {r}, true);
    add("dec/prelu_r/alpha", {r}, true);
    for (int j = 0; j < 2 * L; ++j) {
      int hin, cin, hout, cout, s;
      dec_layer(j, &hin, &cin, &hout, &cout, &s);
      char b[64];
      snprintf(b, sizeof b, "dec/convt%d/kernel", j);
      add(b, {dec_ksz(j), dec_ksz(j), cout, cin}, true);
      snprintf(b, sizeof b, "dec/convt%d/bias", j);
      add(b, {cout}, true);
      snprintf(b, sizeof b, "dec/prelut%d/alpha", j);
      add(b, {hout, hout, cout}, true);
    }
    add("dec/head/kernel", {3, 3, c->filters[0], 2 * C}, true);
    add("dec/head/bias", {2 * C}, true);
    // (any band count 1 .. 7: the first conv reads bands + 1 of 8 folded channels, the head stores 2*bands of C2p
    // columns, and the label / output rows of the head kernels are addressed per element unless bands == 6)
    // flat layout: [encoder trainables | decoder trainables | non-trainables], every tensor 16-byte aligned
    size_t off = 0;
    n_enc_params = n_dec_params = n_trainable_params = 0;
    for (int pass = 0; pass < 3; ++pass) {
      for (size_t i = 0; i < specs.size(); ++i) {
        Spec& s = specs[i];
        bool enc = (int)i < D0;
        int cls = s.trainable ? (enc ? 0 : 1) : 2;
        if (cls != pass) continue;
        s.off = off;
        off += (s.count + 3) & ~(size_t)3;
      }
      if (pass == 0) n_enc_train = off;
      if (pass == 1) n_train = off;
    }
    n_total = off;
    for (size_t i = 0; i < specs.size(); ++i) {
      ((int)i < D0 ? n_enc_params : n_dec_params) += (int64_t)specs[i].count;
      if (specs[i].trainable) n_trainable_params += (int64_t)specs[i].count;
    }
    return OK;
  }

  void macs(int64_t* enc, int64_t* dec) const {
    int64_t e = 0, dd = 0;
    for (int j = 0; j < 2 * L; ++j) {
      int hin, cin, hout, cout, s;
      enc_layer(j, &hin, &cin, &hout, &cout, &s);
      e += (int64_t)hout * hout * enc_ksz(j) * enc_ksz(j) * cin * cout;
    }
    e += (int64_t)flat * tw;
    dd += (int64_t)d * dec_hidden + (int64_t)dec_hidden * w0 * w0 * cfg.filters[L - 1];
    for (int j = 0; j < 2 * L; ++j) {
      int hin, cin, hout, cout, s;
      dec_layer(j, &hin, &cin, &hout, &cout, &s);
      dd += (int64_t)hin * hin * dec_ksz(j) * dec_ksz(j) * cin * cout;  // every input pixel meets all k*k taps
    }
    dd += (int64_t)dec_out * dec_out * 9 * cfg.filters[0] * 2 * C;
    *enc = e;
    *dec = dd;
  }
};

// --------------------------------------------------------------------------------------------
// tap tables
// --------------------------------------------------------------------------------------------
struct Taps {
  int n = 0;
  // legacy 4-bit codes of the 3 x 3 kernel families (gconv2 / strip / Winograd: offsets -1 .. 2, at most 16 taps) ...
  unsigned long long tapcode = 0, wtcode = 0;
  bool legacy = true;      // ... which cannot express this tap set when false
  // ... and the general table (gconv / wgrad kernels, any kernel size up to 5 x 5)
  TapTab xt = {};
  void add(int dh, int dw, int wt) {
    if (n < DV_MAX_TAPS) xt.t[n] = (unsigned)(dh + 8) | ((unsigned)(dw + 8) << 4) | ((unsigned)wt << 8);
    if (n < 16 && dh >= -1 && dh <= 2 && dw >= -1 && dw <= 2 && wt < 16) {
      tapcode |= (unsigned long long)(((dh + 1) & 3) | (((dw + 1) & 3) << 2)) << (4 * n);
      wtcode |= (unsigned long long)(wt & 15) << (4 * n);
    } else {
      legacy = false;
    }
    ++n;
    xt.n = n;
  }
};
// input pixel = out*s + k - pad_before, k x k kernel
static Taps taps_fprop(int pb, int k = 3) {
  Taps t;
  for (int kh = 0; kh < k; ++kh)
    for (int kw = 0; kw < k; ++kw) t.add(kh - pb, kw - pb, kh * k + kw);
  return t;
}
// data-gradient form: target pixel o = s*i~ + ph, source i = i~ + (ph + pb - kh)/s for kh == ph+pb (mod s)
static Taps taps_dgrad(int s, int pb, int ph, int pw, int k = 3) {
  Taps t;
  for (int kh = 0; kh < k; ++kh) {
    int nh = ph + pb - kh;
    if (((nh % s) + s) % s) continue;
    for (int kw = 0; kw < k; ++kw) {
      int nw = pw + pb - kw;
      if (((nw % s) + s) % s) continue;
      // floor division: nh is a multiple of s here, so / is exact
      t.add(nh / s, nw / s, kh * k + kw);
    }
  }
  return t;
}
static int ilog2_exact(int v) {
  for (int s = 0; s < 31; ++s)
    if ((1 << s) == v) return s;
  return -1;
}

}  // namespace dv

// --------------------------------------------------------------------------------------------
// handles
// --------------------------------------------------------------------------------------------
namespace dv {
struct InferPipe;

// The per-stamp tables of a field-sourced job in device memory: the windows' corners, the integer placements (compositing
// calls), the field of every stamp, the first stamp of every field, and the centre MSE the job writes.  One call's locals in
// infer_fields_impl, a resident field set's growable member.
struct StampTables {
  DevBuf<int> starts, places, sfield, fptr;
  DevBuf<double> mse;
  // what a call sets aside for them, whichever of them it fills
  static size_t bytes(size_t N, size_t M) { return N * (5 * sizeof(int) + sizeof(double)) + (M + 1) * sizeof(int); }
  // grows the tables to N stamps (at least min_stamps) of M fields and queues their upload on s; places_h null / want_mse
  // false: the job has no use for that table, it stays as it is
  int upload(int64_t N, int M, const int32_t* starts_h, const int32_t* places_h, const int32_t* sfield_h, const int* fptr_h,
             bool want_mse, size_t min_stamps, hipStream_t s) {
    const size_t n = std::max((size_t)N, min_stamps), sb = (size_t)N * 2 * sizeof(int);
    DV_TRY(starts.ensure(2 * n));
    if (places_h) DV_TRY(places.ensure(2 * n));
    DV_TRY(sfield.ensure(n));
    DV_TRY(fptr.ensure((size_t)M + 1));
    if (want_mse) DV_TRY(mse.ensure(n));
    DV_HIP(hipMemcpyAsync(starts, starts_h, sb, hipMemcpyHostToDevice, s));
    if (places_h) DV_HIP(hipMemcpyAsync(places, places_h, sb, hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(sfield, sfield_h, (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(fptr, fptr_h, ((size_t)M + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    return OK;
  }
};
}

struct dv_ctx {
  int device = 0, rank = 0, world = 1;
  hipStream_t stream = nullptr;
  hipStream_t comm_stream = nullptr;   // gradient all-reduce runs here, overlapped with the encoder backward
  hipStream_t aux_stream = nullptr;    // weight-gradient kernels run here, beside the data-gradient chain
  hipStream_t red_stream = nullptr;    // small d(alpha) / d(bias) reductions (and the H2D copies of the inference pipeline)
  hipEvent_t ev_red = nullptr;
  hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};   // extra forward lanes
  hipEvent_t ev_lane[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_ready = nullptr, ev_join = nullptr, ev_buf[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_dec = nullptr, ev_enc = nullptr, ev_comm = nullptr, ev_small = nullptr, ev_small2 = nullptr;
  hipEvent_t ev_mid = nullptr;
  hipEvent_t ev_wred = nullptr;   // weight-gradient stream -> reduction stream at a bucket boundary of the bf16 backward
  ncclComm_t comm = nullptr;
  // timing of the collectives (dv_comm_prof_*: the multi-rank bench's "comm time vs exposed comm time"): event pairs around
  // every collective on the comm stream, and around the main stream's waits for them
  bool cprof_on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> cprof_comm, cprof_wait;
  std::vector<hipEvent_t> cprof_pool;
  bool fake_peers = false;   // DV_DEBUG_FAKE_PEERS rehearsal: world > 1 but a one-rank communicator (results mean nothing)
  float* red_dev = nullptr;  // small device buffer for host all-reduce
  std::vector<dv_model*> models;   // live models of this context: dv_ctx_destroy destroys them first
};

struct ProfRec {
  int klass;
  int fam;
  hipEvent_t a, b;
};
// kernel families of the MFMA work, by the name rocprofv3 prints for them (per-kernel roofline rows of bench.py)
enum {
  PF_NONE = -1, PF_GCONV2 = 0, PF_GCONV_S2, PF_GSTRIP, PF_GSTRIP8, PF_GCONV, PF_WGRAD, PF_WSTRIP, PF_BCONV, PF_BWGRAD,
  PF_WINO, PF_WINOW, PF_BTRUNK, PF_COUNT
};
static const char* const kProfFamName[PF_COUNT] = {
    "gconv2_kernel", "gconv_s2_kernel", "gconv_strip_kernel", "gconv_strip8_kernel", "gconv_kernel", "wgrad_kernel",
    "wgrad_strip_kernel / wgrad_strip8_kernel", "bconv_kernel", "bwgrad_kernel", "wino_conv4_kernel / wino_conv_kernel", "wino_wgrad_kernel",
    "bgemm_kernel / bgemm_tn_kernel"};

struct DataSlot {
  float* x = nullptr;
  float* y = nullptr;
  int64_t n = 0;
  // streamed slot (dv_data_stream_open): the caller's host rows, gathered per step into the model's StreamRing
  bool streamed = false;
  const char *hx = nullptr, *hy = nullptr;
  bool x64 = false, y64 = false;
  int64_t sx = 0, sy = 0;        // row strides in bytes
  int64_t h2d_bytes = 0;
  // the per-step view of a streamed batch handed to enqueue_step: x / y point into a device ring slot, and every
  // stream that reads them first waits for `ready` (the end of their host-to-device copy)
  hipEvent_t ready = nullptr;
};

// Device ring of a streamed slot (shared by slots 0 and 1: the steps of both are queued in one order).  Entry r holds
// one batch, x rows then y rows (y from yoff), in HBM (dev) and in pinned staging (host).
//
// Hazards.  fit() queues training steps two ahead under tickets 0..3, so up to three steps are in flight when the host
// gathers the next one.  The batch of step k lives in entry k % 4 and is read by:
//   - the comm stream: bn_prefetch's batch statistics and, on the bf16 engine, bf_input into xh_alt, queued at enqueue time
//     ahead of the step's forward (shuffled batches);
//   - the main stream: the fp32 forward's conv0 input (or the statistics / input kernel when nothing was prefetched) and
//     the labels read by the fused head or the head kernel (forward lanes join the main stream);
//   - the weight-gradient (aux) stream: conv0's weight gradient and the input BatchNorm's gradient read x;
//   - the reduction stream, which is recorded as well so that no future change of what it reads opens a race.
// At the end of step k's enqueue a release event is recorded on each of those streams (rel[r][..]): every reader of the
// entry was queued before it.  The copy of step k + 4 into the same entry waits for all of them on the copy stream (which
// nothing else waits on, so these waits stall no compute queue), and every reader of step k + 4 waits for that copy's
// event (h2d[r]): the comm stream before bn_prefetch, the main stream before the forward; the aux and reduction streams
// start a step's work only behind events of the main stream.  The pinned entry is rewritten by the host only after
// h2d[r] has completed (the gather of step k + 4 synchronises on the copy of step k, long finished in steady state).
struct StreamRing {
  static constexpr int kDepth = 4;
  static constexpr int kRel = 4;          // main, aux, comm, reduction stream
  dv::DevBuf<float> dev[kDepth];
  dv::PinBuf<float> host[kDepth];
  size_t yoff = 0;                        // floats from an entry's x rows to its y rows (256-byte aligned)
  hipStream_t copy = nullptr;
  hipEvent_t h2d[kDepth] = {};
  hipEvent_t rel[kDepth][kRel] = {};
  bool queued[kDepth] = {};               // h2d / rel of the entry have been recorded
  unsigned next = 0;
  int threads = 1;
  std::vector<int32_t> iota;              // [0, Bc): index vector of a gathered batch
  ~StreamRing() {                         // (the buffers free themselves)
    for (int r = 0; r < kDepth; ++r) {
      if (h2d[r]) (void)hipEventDestroy(h2d[r]);
      for (auto e : rel[r])
        if (e) (void)hipEventDestroy(e);
    }
    if (copy) (void)hipStreamDestroy(copy);
  }
};

// bf16 kernel family (BASELINE configs[2], bf16.h): stamp-inner bf16 activations of the conv stacks, bf16 weight
// matrices cast from the fp32 master tensors, fp32 dense trunk / sampler / head
struct BfW {
  void* f = nullptr;   // forward form   [Cout][Kf]
  void* d = nullptr;   // data-gradient form [Cin][Kd]
  int Kf = 0, Kd = 0;
};
struct BfState {
  bool on = false;
  // master weights changed since the bf16 matrices were cast, per gradient bucket (bit 0: shallow half of the encoder, 1: deep
  // half - conv L .. dense -, 2: decoder; the descriptors are sorted by bucket).  A bucket that early Adam updates on the
  // comm stream is re-cast right there (bf_cast_bucket), off the main stream; the next forward casts what is left
  unsigned dirty_mask = 7, early_cast = 0;
  int desc_off[4] = {0, 0, 0, 0};
  int NBp = 0;                   // stamps of the current pass padded to 16
  void* xh = nullptr;            // normalised input [HW][NBp][16]
  // Round 6: the input of the NEXT training step is normalised ahead, on the comm stream, into the other of two buffers
  // (bn_prefetch: batch statistics -> bn_finalize -> bf_input; 26 us that used to open every step on the main stream).
  // `xh` is the buffer of the step in flight (its first conv and, at the very end, its first-layer weight gradient read it).
  void* xh_alt = nullptr;
  // head fused into the head conv's epilogue (BEPI_HEAD): forward_all leaves the request before the decoder runs, the head conv
  // takes it when its launch has the row-strip form, head_lane then only reports the number of partial rows
  dv::BHeadFuse hfuse;
  bool tpre_stale = false;       // the last forward pass ran the head in the conv's epilogue: tpre32 was not written
  bool hfuse_req = false;
  long hfuse_tiles = 0;
  bool head_marked = false;      // bf_backward recorded the main stream behind the head kernel: the head's weight gradient waits for that record
  bool in_pre = false;           // xh_alt holds the prefetched batch, bnstate / the moving statistics are already its
  std::vector<void*> enc_u, enc_a, dec_u, dec_a;
  void* dec_in = nullptr;        // decoder trunk output as a stamp-inner tensor [w0*w0][NBp][f_last]
  float* tpre32 = nullptr;       // head conv output, fp32 [Hd*Hd][NBp][16]
  void* dt = nullptr;            // d(loss)/d(tpre), bf16
  float* flat_in = nullptr;      // encoder output as fp32 rows [NB][flat] (input of the flatten PReLU)
  std::vector<void*> du_enc, du_dec;   // where the last backward pass left d(pre-activation) of every conv layer, and
  void* d_dec_in = nullptr;            // d(decoder trunk output) (introspection: dv_model_get_activation "enc_du3" ...)
  std::vector<void*> gpool;      // one activation-gradient buffer per data-gradient launch of a step (bf16): the
                                 // weight gradients run on the aux stream and nothing ever waits for a buffer
  dv::BRedBatch red;             // fused-epilogue partials of the backward pass being queued (summed in two launches)
  float* slab = nullptr;         // weight-gradient partial slabs (aux stream): a per-pass pool, every launch its region
  size_t slab_elems = 0;
  size_t slab_off = 0;
  size_t slab_tail = 0;          // extra region behind the pool for the one launch queued on the main stream (never
                                 // touched by the weight-gradient stream, whose reductions may lag behind the main stream)
  dv::WRedBatch wred;            // their reductions, all in one launch at the end of the pass (bf_flush_wred)
  bool red_pending = false;      // a bucket boundary of this pass queued its slab sums on the REDUCTION stream: the pool must
                                 // not be rewound under them (bf_wgrad's pool-full path waits for that stream first)
  std::vector<BfW> enc_w, dec_w;
  BfW head_w;
  std::vector<dv::BCastDesc> descs;
  dv::BCastDesc* descs_dev = nullptr;
  float* G0s16 = nullptr;        // not used directly: slabs of the first layer reduce into G0s
  float *wx32 = nullptr, *wy32 = nullptr;   // fp32 [NB][pixels * channels] copies of the two operands of a weight gradient whose
                                 // kernel size is not 3 (the bf16 weight-gradient kernel holds nine taps): see bf_wgrad_f32
  void* zero = nullptr;          // 1 KiB of zeros
  float* trunk[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // fp32 gradient rows of the dense trunk, one buffer per
                                 // stage of a backward pass (its weight gradients read them from the aux stream)
  // ---- dense trunk on the bf16 matrix cores (btrunk.hip, round 6): the two large Dense layers (flatten -> params_size,
  // 560 -> w*w*f) and their data / kernel gradients as bf16-MFMA products that read and write the stamp-inner tensors of
  // the conv stacks directly.  On when the last encoder level has a multiple of 64 filters (the 59-px and 128-px nets);
  // other geometries keep the fp32 trunk between two layout conversions (DV_BF_TRUNK=0 forces that form for an A/B).
  bool trunk_mfma = false;
  int FL = 0, TWn = 0, TWk = 0, HIDn = 0, HIDk = 0;   // flat; params_size padded to 32 (as N) / 64 (as K); 560 likewise
  void *wenc_f = nullptr, *wenc_d = nullptr;          // encoder Dense kernel: [TWn][FL] (forward), [FL][TWk] (data gradient)
  void *w1_f = nullptr, *w1_d = nullptr;              // decoder Dense 560 -> flat: [FL][HIDk] (forward), [HIDn][FL] (data gradient)
  float* tslab = nullptr;                             // K-split partial sums [<= 8][Bp][max(TWn, HIDn)]
  int t_nslab = 0;                                    // > 0: m->t is still these slabs + bias (the sampler, or bf_finish_t, adds them)
  void* dec_ur = nullptr;                             // bf16 stamp-inner pre-activation of the decoder trunk's output
};

// Winograd-domain weights of one stride-1 3x3 layer in one form (forward or data gradient), see wino.hip
struct WinoEntry {
  dv::WinoWDesc d;
  uint64_t epoch = ~(uint64_t)0;   // parameter epoch the transform was computed at
};

// a resident field set (dv_field_set_*), owned by its model
struct dv_field_set {
  dv_model* m = nullptr;
  int M = 0, F = 0, nb = 0;
  bool cumulative = false, open = false;
  // [M][F][F][nb] each.  reference mode: base, work, next, fin, mean, stddev; cumulative mode: `fin` is `work` and `base` is
  // not kept (every pass starts from the working residual).  `next` receives a pass's new working residual while the
  // pass's later chunks still gather from `work`.
  dv::DevBuf<double> base, work, next, fin, mean, stddev;
  dv::DevBuf<double> mse_part, fmse;             // partial sums and results of the field_mse reduction
  // the detector's weight planes [M][F][F] (dv_field_set_detect_weights): while held, dv_field_set_detect
  // takes the weighted path with dnoise / dfilter
  dv::DevBuf<double> dweights;
  int dnoise = 0, dfilter = 0;
  // the detector's band selection (dv_field_set_detect_bands): while dbands is not empty, dv_field_set_detect
  // takes the multi-band path with the c_j in dbw, the planes [M][F][F][k] in dplanes (if any) and dbnoise / dbfilter
  std::vector<int32_t> dbands;
  std::vector<double> dbw;
  dv::DevBuf<double> dplanes;
  int dbnoise = 0, dbfilter = 0;
  // the object columns of the last detection (dv_field_set_detect_objects), on the host: while dobj is set
  // dv_field_set_detect asks for them (dseg: and for the segmap [M][F][F]); do_n rows are held, -1: none
  bool dobj = false, dseg = false;
  int64_t do_n = -1;
  std::vector<int32_t> do_i[dv::DET_OBJ_I], do_seg;
  std::vector<double> do_d[dv::DET_OBJ_D];
  // the cleaning pass (dv_field_set_detect_clean): while dclean is set dv_field_set_detect runs it with
  // dclean_param and the set keeps the clean columns of its last detection on the host: dc_n rows (-1: none), dc_nraw [M]
  bool dclean = false;
  double dclean_param = 1.0;
  int64_t dc_n = -1;
  std::vector<int32_t> dc_nmerged;
  std::vector<double> dc_mthresh;
  std::vector<int64_t> dc_nraw;
  dv::StampTables tab;                         // the per-stamp tables of a pass, kept between passes and grown on demand
  std::vector<double> fmse_h;                     // host side of fmse
  // the catalogue of the measured passes (dv_field_set_pass_measure).  Resident rows: {shape[5], status,
  // place, field} of every stamp of every pass that took child sums, in call order; nrows of them are kept, the tail up
  // to rcap is where the running pass measures.  The other columns of a pass leave with it: per-pass buffers.
  dv::DevBuf<double> rshape, rsums;              // [rcap][5]; [nrows][4]: the sums of dv_field_set_blend
  dv::DevBuf<int> rstatus, rplaces, rfield;      // [rcap], [rcap][2], [rcap]
  size_t nrows = 0, rcap = 0;
  dv::DevBuf<double> cflux, cferr, cblend;       // [N][nb], [N][nb], [N][4] of the running pass
  dv::DevBuf<int> citers, cnpix;                 // [N]
  // room for `need` resident rows: a larger set of buffers takes the kept rows over on s (the old ones go once s is idle)
  int rows_reserve(size_t need, hipStream_t s) {
    if (need <= rcap) return dv::OK;
    const size_t cap = std::max<size_t>({need, 2 * rcap, 1024});
    dv::DevBuf<double> sh;
    dv::DevBuf<int> st, pl, fi;
    DV_TRY(sh.alloc(cap * 5));
    DV_TRY(st.alloc(cap));
    DV_TRY(pl.alloc(cap * 2));
    DV_TRY(fi.alloc(cap));
    if (nrows > 0) {
      DV_HIP(hipMemcpyAsync(sh, rshape, nrows * 5 * sizeof(double), hipMemcpyDeviceToDevice, s));
      DV_HIP(hipMemcpyAsync(st, rstatus, nrows * sizeof(int), hipMemcpyDeviceToDevice, s));
      DV_HIP(hipMemcpyAsync(pl, rplaces, nrows * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
      DV_HIP(hipMemcpyAsync(fi, rfield, nrows * sizeof(int), hipMemcpyDeviceToDevice, s));
      DV_HIP(hipStreamSynchronize(s));
    }
    rshape = std::move(sh);
    rstatus = std::move(st);
    rplaces = std::move(pl);
    rfield = std::move(fi);
    rcap = cap;
    return dv::OK;
  }
  // the stamp store of the joint flux fit (dv_field_set_keep_stamps): with `keep` on, a pass that keeps resident
  // rows also keeps its float32 mean stamps, each at its resident row number, and the host remembers the pass's field_ptr and
  // placements - what dv_field_set_fit_flux regroups field by field
  bool keep = false;
  dv::DevBuf<float> rstamps;                     // [scap][cs][cs][nb]
  size_t scap = 0;
  std::vector<std::vector<int>> pass_fptr;       // per kept pass: the first row of every field, counted from the pass's row 0
  std::vector<int32_t> places_h;                 // [nrows][2]: the host's copy of rplaces
  // room for the stamps of `need` resident rows of `stamp` floats: grows like rows_reserve, the kept stamps copied over on s
  int stamps_reserve(size_t need, size_t stamp, hipStream_t s) {
    if (need <= scap) return dv::OK;
    const size_t cap = std::max<size_t>({need, 2 * scap, 1024});
    dv::DevBuf<float> st;
    DV_TRY(st.alloc(cap * stamp));
    if (nrows > 0) {
      DV_HIP(hipMemcpyAsync(st, rstamps, nrows * stamp * sizeof(float), hipMemcpyDeviceToDevice, s));
      DV_HIP(hipStreamSynchronize(s));
    }
    rstamps = std::move(st);
    scap = cap;
    return dv::OK;
  }
};

static void field_set_release(dv_field_set* fs) {
  for (dv::DevBuf<double>* b : {&fs->base, &fs->work, &fs->next, &fs->fin, &fs->mean, &fs->stddev, &fs->mse_part, &fs->fmse,
                                &fs->dweights, &fs->dplanes, &fs->rshape, &fs->rsums, &fs->cflux, &fs->cferr, &fs->cblend})
    b->reset();
  for (dv::DevBuf<int>* b : {&fs->rstatus, &fs->rplaces, &fs->rfield, &fs->citers, &fs->cnpix}) b->reset();
  fs->nrows = fs->rcap = 0;
  fs->rstamps.reset();
  fs->scap = 0;
  fs->pass_fptr.clear();
  fs->places_h.clear();
  fs->tab = dv::StampTables();
  fs->open = false;
}

struct dv_model {
  dv_ctx* ctx = nullptr;
  dv::Arch A;
  std::vector<WinoEntry> wino;     // (W, nmajor, tap map) -> transformed weights
  dv::WinoWDesc* wino_descs_dev = nullptr;
  size_t wino_descs_cap = 0;
  uint64_t param_epoch = 0;        // bumped whenever a parameter changes (Winograd weights are re-derived lazily)
  bool use_wino = true;
  std::vector<std::pair<float*, size_t>> wino_wslabs;   // partial-slab buffer of the i-th Winograd weight-gradient launch of a step
  int wino_wcount = 0;
  int Bc = 0;
  BfState bf;
  // flat parameter-shaped buffers
  float *P = nullptr, *G = nullptr, *Mm = nullptr, *Vv = nullptr;
  float* W1p = nullptr;  // first conv kernel with the input BatchNorm folded in, 8 input channels
  float* G0s = nullptr;  // gradient w.r.t. W1p (scratch)
  float *Whp = nullptr, *bhp = nullptr, *Ghs = nullptr;  // head kernel/bias padded to C2p output channels, grad scratch
  // latent sizes that are not multiples of 4 (model.py:164 takes any latent_dim): the encoder's Dense kernel / bias with their
  // tw columns padded to twp (zeros), the decoder's first Dense kernel with its d rows padded to dp (zeros), and the scratch
  // their weight gradients are written to; null when no padding is needed
  float *Wdp = nullptr, *bdp = nullptr, *Gdp = nullptr, *W0p = nullptr, *G0p = nullptr;
  bool enc_trainable = true, dec_trainable = true;
  bool opt_enc = true, opt_dec = true;  // what the current optimizer updates (fixed at dv_optimizer_reset)
  float lr = 1e-4f, b1 = 0.9f, b2 = 0.999f, aeps = 1e-7f;
  int64_t iter = 0;
  // activations
  float* xn = nullptr;
  std::vector<float*> enc_u, enc_a, dec_u, dec_a;
  std::vector<float*> du_enc, du_dec;   // where the last backward pass left d(pre-activation) of every conv layer (the
                                        // per-step buffer pool keeps them until the next pass; tests/test_gpu_layers.py)
  bool du_valid = false;
  float* da_enc0 = nullptr;
  float *flat_a = nullptr, *t = nullptr, *eps = nullptr, *z = nullptr, *zstd = nullptr, *kl = nullptr;
  float *dec_ain = nullptr, *dec_uh = nullptr, *dec_ah = nullptr, *dec_ur = nullptr, *dec_ar = nullptr;
  bool ain_done = false;   // the sampler launch of this pass has already written dec_ain = PReLU(z) (model.py:113)
  float *tpre = nullptr, *loc = nullptr, *scale = nullptr;
  float *gA = nullptr, *gB = nullptr, *gC = nullptr;
  float* ws4 = nullptr;  // split-K slabs of the dense layers (ws1 belongs to the weight-gradient stream)
  float* arena = nullptr;  // per-step bump arena for d(alpha)/d(bias) partials reduced on the aux stream
  size_t arena_elems = 0, arena_off = 0;
  size_t ws4_elems = 0;
  hipStream_t wstream = nullptr;  // stream the weight-gradient kernels are queued on (aux or main)
  hipStream_t cs = nullptr;       // stream of the forward lane being queued (null: main stream)
  int b0 = 0;                     // first stamp of the forward lane being queued
  int lane_id = 0;
  bool split_forward = true;      // forward lanes allowed (DV_NO_FWD_SPLIT forbids them; DV_FWD_LANES=n asks for n)
  bool overlap_wgrad = true;
  bool fuse_first = true;     // DV_NO_FUSE_FIRST=1 keeps the first PReLU backward as a separate pass
  bool no_fuse = true;        // dv_debug_fuse_prelu_bwd(1) fuses the PReLU backward into the data-gradient epilogue (batch-major
                              // tiles); measured 3 % slower than the separate pass on MI355X (scattered 128-byte rows), so off
  bool arena_reduce = true;   // queue d(alpha)/d(bias) reductions on the aux stream (off with DV_NO_OVERLAP)
  float *ws1 = nullptr, *ws2 = nullptr, *ws3 = nullptr;
  size_t ws1_elems = 0, ws2_elems = 0, ws3_elems = 0;
  float *scal = nullptr, *bnstate = nullptr, *bnsums = nullptr;
  float* stage_x = nullptr;  // host-batch staging (infer / encode)
  dv::InferPipe* pipe = nullptr;
  std::vector<dv_field_set*> field_sets;   // every set opened on this model, closed ones included: freed with the model
  // deferred step results (dv_train_step_async / dv_step_result): pinned scalars and staged indices per ticket
  float* ring_scal = nullptr;    // [4][4] pinned
  int* ring_idx = nullptr;       // [4][Bc] pinned
  hipEvent_t ring_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int ring_bg[4] = {0, 0, 0, 0};
  bool ring_used[4] = {false, false, false, false};
  // input-BN batch sums of the NEXT step, computed (and all-reduced) on the comm stream while this step runs
  float* bn_pre_part = nullptr;
  float* bn_pre_sums = nullptr;
  size_t bn_pre_part_elems = 0;
  bool bn_pre_valid = false;
  bool bnpre_go_pending = false;   // bf16 engine: ev_bnpre_go is recorded behind the input kernel of this forward pass
  const float* bn_pre_x = nullptr;
  const int* bn_pre_idx = nullptr;   // device index vector the prefetched sums belong to (null: contiguous rows)
  int* idx_slots = nullptr;          // [4][Bc] device index vectors of queued train steps (filled on the comm stream)
  unsigned idx_slot_next = 0;
  int64_t bn_pre_first = -1, hint_next_first = -1;
  int bn_pre_B = 0;
  hipEvent_t ev_bnpre = nullptr, ev_bnpre_go = nullptr;
  // weight-gradient partial slabs rotate through three regions of ws1 so that a layer's slab reduction (reduction
  // stream) can run beside the next layer's weight-gradient kernel (aux stream)
  int ws_region = 0;
  bool ws_pending[3] = {false, false, false};
  hipEvent_t ev_wk[3] = {nullptr, nullptr, nullptr}, ev_rk[3] = {nullptr, nullptr, nullptr};
  int ws_last = -1;              // region whose reduction produced the most recent weight gradient
  // "no reuse" mode (allocated at the first overlapped backward, DV_NO_STEP_POOL=1 keeps the rotating form): every
  // data-gradient launch of a step gets its own output buffer and every weight-gradient launch its own slab region,
  // so that neither stream has to wait for the other to release one - each such wait, even on a long-completed
  // event, costs its queue ~5 us (a barrier packet), ~40 of them per step
  std::vector<float*> gbufs;     // [0..2] = gA, gB, gC, then the pool
  float* gpool = nullptr;
  float* ws1x = nullptr;
  int ws_nreg = 3;               // slab regions: 3 (rotating, with waits) or one per launch of a step
  size_t ws_region_cap = 0;
  int ws_count = 0;              // weight-gradient launches of this step so far
  // bf16 train / gradient steps with a reduction stream: the loss sums (and the head's bias column sums) are queued there
  // at the start of the backward pass instead of on the main stream between the two passes (bf_backward)
  float* ws_head = nullptr;      // head partials of such a step (ws3 stays the main stream's)
  bool defer_loss_sums = false, loss_pending = false;
  int loss_blocks = 0, loss_NB = 0;
#ifdef DV_DEBUG_EXPORTS
  std::vector<std::function<int()>> exp_deferred;   // DV_EXP_DEFER_WGRAD (MEASUREMENT only): launches held back for the next forward pass
#endif
  hipStream_t ws_last_rs = nullptr;
  bool step_pool_tried = false;
  size_t max_act_elems = 0;      // Bc * largest per-stamp activation
  bool main_marked = false;      // ev_ready was recorded on the main stream right behind its last kernel
  // small-batch inference (~45 kernels of a few microseconds), opt-in: the forward of a batch size is captured into a
  // hipGraph at its second use and replayed afterwards; the noise seed lives in device memory
  unsigned long long* seed_dev = nullptr;
  bool use_seed_dev = false;
  bool infer_graph = false;      // dv_config.infer_graph
  uint64_t graph_epoch = ~(uint64_t)0;   // parameter epoch the captured graphs belong to
  // set by dv_infer / dv_encode / dv_decode for calls of at most 16 stamps: the deep layers slice K over workgroups
  // (gconv2_small_splitk).  Decided per CALL, not per launch, so that how a longer input is chunked never changes bits.
  bool tiny_call = false;
  bool keep_outputs = false;     // gradient / train steps also write loc and scale (introspection)
  std::map<int, hipGraphExec_t> infer_graphs;
  std::map<int, int> infer_seen;
  bool normalise = false;        // dv_model_set_normalise: tanh(arcsinh) on inference inputs, inverse on the mean
  bool mse_sample = false;       // dv_model_set_mse_sample: DV_S_MSE against a sample of the output distribution
  unsigned long long cur_seed = 0;   // noise seed of the pass being queued
  bool early_adam = false;       // this step updates finished parameter ranges on the comm stream while the backward runs
  float lr_t_step = 0.f;         // bias-corrected step size of this step
  size_t adam_done_from = 0;     // ranges [adam_done_from, n_train) have been updated already (this step)
  size_t enc_reduced_from = 0;   // this step's encoder gradients [enc_reduced_from, n_enc_train) are already all-reduced   // pinned staging + copy streams of the pipelined dv_infer (lazy)
  float* zero_page = nullptr;  // 256 B of zeros (LDS-DMA source for out-of-image pieces)
  int* idx_dev = nullptr;
  DataSlot slots[2];
  StreamRing* ring = nullptr;    // allocated by the first dv_data_stream_open, freed when no slot streams any more
  int lastB = 0;
  // profiling
  bool prof_on = false;
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  int64_t prof_n[3] = {0, 0, 0};
  int64_t prof_launches[3] = {0, 0, 0};
  bool prof_open = false;
  int prof_open_fam = -1;
  int64_t fam_launches[16] = {0};
  double fam_ms[16] = {0}, fam_flops[16] = {0}, fam_exec[16] = {0}, fam_bytes[16] = {0};
  int prof_open_klass = 0;
  hipStream_t prof_open_stream = nullptr;
  hipEvent_t prof_open_ev = nullptr;
  double prof_ms[3] = {0, 0, 0};
  std::vector<void*> allocs;
};

namespace dv {

static int dalloc(dv_model* m, float** p, size_t elems) {
  void* q = nullptr;
  if (elems == 0) elems = 4;
  hipError_t e = hipMalloc(&q, elems * sizeof(float));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
  m->allocs.push_back(q);
  *p = (float*)q;
  return OK;
}

// Per-class HIP-event timing.  Consecutive launches of one class on one stream share a single event pair (the
// pair brackets the whole run, inter-kernel boundaries included), so that the events themselves add little.
static hipEvent_t prof_event(dv_model* m) {
  hipEvent_t e;
  if (!m->ev_pool.empty()) {
    e = m->ev_pool.back();
    m->ev_pool.pop_back();
  } else {
    (void)hipEventCreate(&e);
  }
  return e;
}
static void prof_close(dv_model* m) {
  if (!m->prof_open) return;
  hipEvent_t b = prof_event(m);
  (void)hipEventRecord(b, m->prof_open_stream);
  m->prof.push_back({m->prof_open_klass, m->prof_open_fam, m->prof_open_ev, b});
  m->prof_open = false;
}
struct ProfScope {
  // fam / flops: kernel family of an MFMA launch and its algorithmic FLOPs (padding taps counted);
  // exec: the FLOPs the matrix pipe EXECUTES for it (< 0: the algorithmic ones) - a Winograd launch executes 16 multiplies
  // per 2 x 2 tile and channel pair instead of 36, over blocks / column tiles padded to the kernel's geometry;
  // bytes: algorithmic HBM bytes of the launch (operands read once, results written once)
  ProfScope(dv_model* m, int k, hipStream_t s = nullptr, int fam = PF_NONE, double flops = 0.0, double exec = -1.0,
            double bytes = 0.0) {
    if (!m->prof_on) return;
    hipStream_t st = s ? s : (m->cs ? m->cs : m->ctx->stream);
    m->prof_launches[k] += 1;
    if (fam >= 0) {
      m->fam_launches[fam] += 1;
      m->fam_flops[fam] += flops;
      m->fam_exec[fam] += exec < 0 ? flops : exec;
      m->fam_bytes[fam] += bytes;
    }
    if (m->prof_open && m->prof_open_klass == k && m->prof_open_fam == fam && m->prof_open_stream == st) return;   // extend the open run
    prof_close(m);
    m->prof_open_ev = prof_event(m);
    (void)hipEventRecord(m->prof_open_ev, st);
    m->prof_open = true;
    m->prof_open_klass = k;
    m->prof_open_fam = fam;
    m->prof_open_stream = st;
  }
};

// a launcher declined the launch (returned 1: geometry not supported) after its ProfScope had counted it
static void prof_uncount(dv_model* m, int k, int fam, double flops, double exec = -1.0, double bytes = 0.0) {
  if (!m->prof_on) return;
  m->prof_launches[k] -= 1;
  if (fam >= 0) {
    m->fam_launches[fam] -= 1;
    m->fam_flops[fam] -= flops;
    m->fam_exec[fam] -= exec < 0 ? flops : exec;
    m->fam_bytes[fam] -= bytes;
  }
}

static int prof_flush(dv_model* m) {
  prof_close(m);
  if (m->prof.empty()) return OK;
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  for (auto& r : m->prof) {
    float ms = 0.f;
    DV_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    m->prof_ms[r.klass] += ms;
    if (r.fam >= 0) m->fam_ms[r.fam] += ms;
    m->ev_pool.push_back(r.a);
    m->ev_pool.push_back(r.b);
  }
  for (int k = 0; k < 3; ++k) {
    m->prof_n[k] += m->prof_launches[k];
    m->prof_launches[k] = 0;
  }
  m->prof.clear();
  return OK;
}


static bool g_force_v1 = false;  // tuning aid: route everything through the first-generation kernel
static bool g_no_special = false; // cross-check aid: skip the strip / fused stride-2 kernels (general gconv2 path only)
static bool g_no_wino = false;    // cross-check aid: stride-1 layers take the direct (strip / gather-GEMM) kernels

// Every collective of a context is issued on ONE stream (comm_stream), the usual single-stream-per-communicator
// pattern; the main stream hands data over and takes it back through events.
// wait = false: the main stream does not wait for the result (the caller joins the comm stream later anyway).
static hipEvent_t cprof_event(dv_ctx* c) {
  hipEvent_t e = nullptr;
  if (!c->cprof_pool.empty()) {
    e = c->cprof_pool.back();
    c->cprof_pool.pop_back();
  } else {
    (void)hipEventCreate(&e);          // timing enabled
  }
  return e;
}
// one all-reduce on the comm stream (every collective of the engine goes through here)
static int comm_allreduce(dv_ctx* c, float* buf, size_t n) {
  hipEvent_t a = nullptr;
  if (c->cprof_on) {
    a = cprof_event(c);
    DV_HIP(hipEventRecord(a, c->comm_stream));
  }
  DV_NCCL(ncclAllReduce(buf, buf, n, ncclFloat, ncclSum, c->comm, c->comm_stream));
  if (a) {
    hipEvent_t b = cprof_event(c);
    DV_HIP(hipEventRecord(b, c->comm_stream));
    c->cprof_comm.push_back({a, b});
  }
  return OK;
}
// the main stream waits for `ev` (recorded on the comm stream behind a collective): with comm profiling the wait is
// bracketed by two timed events - what it costs the main stream is the EXPOSED part of the communication
static int main_waits_for_comm(dv_ctx* c, hipEvent_t ev) {
  hipEvent_t a = nullptr;
  if (c->cprof_on) {
    a = cprof_event(c);
    DV_HIP(hipEventRecord(a, c->stream));
  }
  DV_HIP(hipStreamWaitEvent(c->stream, ev, 0));
  if (a) {
    hipEvent_t b = cprof_event(c);
    DV_HIP(hipEventRecord(b, c->stream));
    c->cprof_wait.push_back({a, b});
  }
  return OK;
}
static int allreduce_small(dv_ctx* c, float* buf, size_t n, bool wait = true) {
  if (!c->comm) return OK;
  DV_HIP(hipEventRecord(c->ev_small, c->stream));
  DV_HIP(hipStreamWaitEvent(c->comm_stream, c->ev_small, 0));
  DV_TRY(comm_allreduce(c, buf, n));
  if (wait) {
    DV_HIP(hipEventRecord(c->ev_small2, c->comm_stream));
    DV_TRY(main_waits_for_comm(c, c->ev_small2));
  }
  return OK;
}

// ---- layer launch helpers ---------------------------------------------------------------------
static void fill_gconv_common(GConvParams& p, const Taps& t, int cin) {
  p.ntaps = t.n;
  p.xt = t.xt;
  p.K = t.n * cin;
  p.cin_shift = ilog2_exact(cin);
}

// Flags of the engine's ordering events.  By default a HIP event record carries a system-scope release (cache write-back
// so that the host and peer GPUs see the data).
//  * One rank (the headline configuration): every event orders streams of ONE GPU - main / aux / reduction / comm
//    stream, forward lanes, buffer hand-overs - whose waiters read through the same L2; results reach the host through
//    copies and the events of the result ring.  The fence is switched off (+0.7 % steps/s; tools/determinism_probe.py
//    stays bit-identical over repeated gradient and train steps).
//  * Several ranks: EVERY event keeps HIP's default system-scope release.  RCCL kernels read the gradient buckets through
//    peer mappings over xGMI and hand results back to the main stream (ev_comm, ev_small2, ev_bnpre); which of those
//    hand-overs could do without the fence has never been measured on more than one GPU (no multi-GPU box is reachable
//    from a build session), so nothing is relaxed there.  DV_EVENT_SCOPE=relaxed opts a multi-rank job into the
//    single-rank flags for exactly that experiment (compare parameters bit for bit against the default).
//  * DV_EVENT_SCOPE=system / device force system scope / an explicit device-scope release everywhere.
static bool g_fuse_prelu_bwd = false;   // dv_debug_fuse_prelu_bwd
static bool g_multi_rank = false;      // set by dv_ctx_create (one context per process) before any event exists
static unsigned sync_event_flags() {
  const char* e = getenv("DV_EVENT_SCOPE");
  if (e && !strcmp(e, "system")) return (unsigned)hipEventDisableTiming;
  if (e && !strcmp(e, "device")) return (unsigned)(hipEventDisableTiming | hipEventReleaseToDevice);
  if (g_multi_rank && !(e && !strcmp(e, "relaxed"))) return (unsigned)hipEventDisableTiming;
  return (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
}
// Events the COMM stream waits on in front of an RCCL launch (gradient buckets, BN sums, loss sums): what is recorded
// behind them is read by OTHER GPUs, so with several ranks they keep the system-scope release even under
// DV_EVENT_SCOPE=relaxed.
static unsigned comm_gate_event_flags() {
  if (g_multi_rank) return (unsigned)hipEventDisableTiming;
  return sync_event_flags();
}

static inline hipStream_t fwd_stream(dv_model* m) { return m->cs ? m->cs : m->ctx->stream; }

// Optional fusion of the PReLU backward of the layer whose OUTPUT gradient a data-gradient launch produces:
// the epilogue turns d(activation) into d(pre-activation) and reduces d(alpha) / d(bias) over the stamps of its
// (batch-major) tile, so the separate prelu_bwd pass over that tensor disappears.
struct FuseBwd {
  const float* u;     // pre-activation of the target layer
  int alpha_spec, bias_spec;
  bool want_grads;    // false: frozen layer, only d(pre-activation) is needed
  // debug harness (no Arch): explicit pointers instead of the spec indices
  const float* alpha_ptr = nullptr;
  float* dalpha_out = nullptr;
  float* dbias_out = nullptr;
};

static int fuse_setup(dv_model* m, GConv2Params& q, const FuseBwd* fz, long* db_rows) {
  const Arch& A = m->A;
  int bm, wgm;
  long mtiles;
  gconv2_tile_geometry(q, &bm, &wgm, &mtiles);
  if (q.NB % bm) return 1;                       // tiles would straddle pixels: caller keeps the separate pass
  q.batch_major = 1;
  q.epi = 3;
  q.Uin = fz->u;
  q.alpha = m->P + A.specs[fz->alpha_spec].off;
  q.alpha_elems = (long)q.Hout * q.Wout * q.Cout;
  q.dal_part = nullptr;
  q.db_part = nullptr;
  *db_rows = mtiles * wgm;
  if (fz->want_grads) {
    const size_t slots = (size_t)(q.NB / bm) * wgm;
    const size_t need = slots * q.alpha_elems + (size_t)(*db_rows) * q.Cout;
    if (m->arena_off + need > m->arena_elems) return 1;
    q.dal_part = m->arena + m->arena_off;
    m->arena_off += slots * q.alpha_elems;
    q.db_part = m->arena + m->arena_off;
    m->arena_off += (size_t)(*db_rows) * q.Cout;
  }
  return OK;
}

static int fuse_finish(dv_model* m, const GConv2Params& q, const FuseBwd* fz, long db_rows) {
  if (!fz->want_grads) return OK;
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  hipStream_t rs = (m->arena_reduce && m->wstream && m->wstream != s) ? m->ctx->red_stream : s;
  if (rs != s) {
    DV_HIP(hipEventRecord(m->ctx->ev_ready, s));
    DV_HIP(hipStreamWaitEvent(rs, m->ctx->ev_ready, 0));
  }
  int bm, wgm;
  long mtiles;
  gconv2_tile_geometry(q, &bm, &wgm, &mtiles);
  const int slots = (q.NB / bm) * wgm;
  ProfScope ps(m, 2, rs);
  DV_TRY(launch_reduce_partials(q.dal_part, m->G + A.specs[fz->alpha_spec].off, slots, q.alpha_elems, 4, 1, 1, rs));
  return launch_reduce_rows_f64(q.db_part, (int)db_rows, q.Cout, m->G + A.specs[fz->bias_spec].off, 1.0f, rs);
}

// Tiny batches (deblend on a few stamps, deblender.py:18): a deep layer has a handful of output tiles, each walking the
// whole K = taps x Cin loop serially at the latency of its own gathers (56 us for the 4 x 4 x 256 layer of one stamp,
// DESIGN 7a).  Slice K over blockIdx.y into raw slabs like the dense layers do and finish with bias + PReLU in
// splitk_finish.  Returns 1 when it handled the launch, 0 when the caller should launch as usual, < 0 on error.
static int gconv2_small_splitk(dv_model* m, GConv2Params& q, int NB, int Hout, int Cout, int nchunks, int epi,
                               const float* bias, const float* alpha, float* U, float* Aout, double flops) {
  if (!m->tiny_call || NB > 16 || q.nclass < 1 || !m->ws4 || m->prof_on || epi > 2) return 0;
  const long M = (long)NB * Hout * Hout;
  const long MN = M * Cout;
  const long tiles64 = ((M + 63) / 64) * (long)((Cout + 63) / 64);
  if (tiles64 > 64 || nchunks < 16 || (MN & 3) || (Cout & 3)) return 0;
  const size_t ws4_cap = m->ws4_elems / 4;
  float* ws4 = m->ws4 + (size_t)m->lane_id * ws4_cap;
  int ks = (int)std::min<long>(std::min<long>(16, nchunks / 4), (long)(ws4_cap / (size_t)MN));
  ks = (int)std::min<long>(ks, std::max<long>(1, 512 / tiles64));
  if (ks < 2) return 0;
  q.ksplit = ks;
  q.U = ws4;
  q.A = nullptr;
  q.epi = 0;
  q.bias = nullptr;
  q.alpha = nullptr;
  {
    ProfScope ps(m, 0, nullptr, PF_GCONV2, flops);
    DV_TRY(launch_gconv2(q, fwd_stream(m)));
  }
  ProfScope ps(m, 2);
  DV_TRY(launch_splitk_finish(ws4, ks, MN, Cout, epi >= 1 ? bias : nullptr, epi == 2 ? alpha : nullptr,
                              (long)Hout * Hout * Cout, U, epi == 2 ? Aout : nullptr, fwd_stream(m)));
  return 1;
}

// ---- Winograd-domain weights (wino.hip) -----------------------------------------------------------------------------
// One entry per (weight tensor, orientation, tap map).  The transform U = G g G^T is re-derived when the parameter
// epoch has moved: for every registered entry in ONE launch at the head of a forward pass (wino_refresh_all, before
// the forward lanes split), or for a single entry at its first use (the debug harness, layers registered late).
static WinoEntry* wino_find(dv_model* m, const float* W, bool nmajor, const Taps& tp) {
  int wtmap[9];
  for (int t = 0; t < 9; ++t) {
    const int dh = (int)((tp.tapcode >> (4 * t)) & 3) - 1, dw = (int)((tp.tapcode >> (4 * t + 2)) & 3) - 1;
    wtmap[(dh + 1) * 3 + (dw + 1)] = (int)((tp.wtcode >> (4 * t)) & 15);
  }
  for (auto& e : m->wino)
    if (e.d.W == W && e.d.nmajor == (nmajor ? 1 : 0) && !memcmp(e.d.wtmap, wtmap, sizeof wtmap)) return &e;
  return nullptr;
}
static int wino_register(dv_model* m, const float* W, bool nmajor, const Taps& tp, int Cin, int Cout, WinoEntry** out) {
  WinoEntry e;
  memset(&e.d, 0, sizeof e.d);
  e.d.W = W; e.d.Cin = Cin; e.d.Cout = Cout; e.d.nmajor = nmajor ? 1 : 0;
  for (int t = 0; t < 9; ++t) {
    const int dh = (int)((tp.tapcode >> (4 * t)) & 3) - 1, dw = (int)((tp.tapcode >> (4 * t + 2)) & 3) - 1;
    e.d.wtmap[(dh + 1) * 3 + (dw + 1)] = (int)((tp.wtcode >> (4 * t)) & 15);
  }
  DV_TRY(dalloc(m, &e.d.Ut, wino_weight_floats(Cin, Cout)));
  m->wino.push_back(e);
  if (out) *out = &m->wino.back();
  return OK;
}
static int wino_upload_descs(dv_model* m, hipStream_t st) {
  if (m->wino_descs_cap < m->wino.size()) {
    float* q = nullptr;
    const size_t cap = m->wino.size() + 16;
    DV_TRY(dalloc(m, &q, (cap * sizeof(WinoWDesc) + 3) / 4));
    m->wino_descs_dev = reinterpret_cast<WinoWDesc*>(q);
    m->wino_descs_cap = cap;
  }
  std::vector<WinoWDesc> h(m->wino.size());
  for (size_t i = 0; i < h.size(); ++i) h[i] = m->wino[i].d;
  DV_HIP(hipMemcpyAsync(m->wino_descs_dev, h.data(), h.size() * sizeof(WinoWDesc), hipMemcpyHostToDevice, st));
  DV_HIP(hipStreamSynchronize(st));          // (h goes out of scope; registration time only)
  return OK;
}
static int wino_refresh_all(dv_model* m, hipStream_t st) {
  if (m->wino.empty()) return OK;
  bool stale = false;
  for (auto& e : m->wino) stale = stale || e.epoch != m->param_epoch;
  if (!stale) return OK;
  std::vector<WinoWDesc> h(m->wino.size());
  for (size_t i = 0; i < h.size(); ++i) h[i] = m->wino[i].d;
  ProfScope ps(m, 2, st);
  DV_TRY(launch_wino_weights(m->wino_descs_dev, h.data(), (int)h.size(), st));
  for (auto& e : m->wino) e.epoch = m->param_epoch;
  return OK;
}
// stride-1, pad-1, nine-tap layer through the Winograd kernel; returns 1 when the layer is not taken
static int wino_conv(dv_model* m, const float* X, const float* W, bool nmajor, const Taps& tp, const float* bias,
                     const float* alpha, float* U, float* Aout, int epi, int NB, int H, int Cin, int Cout, double flops) {
  if (!m->use_wino || g_no_wino || m->tiny_call || m->bf.on || !m->zero_page || !wino_supported(NB, H, Cin, Cout)) return 1;
  // the head conv (16 output columns, or 16 input channels in its data gradient) is faster in strip form: half of the
  // kernel's 32-column tile / 16-channel chunk pipeline would be padding (tools/wino_check.py: 163 vs 114 us)
  if (Cin < 32 || Cout < 32) return 1;
  WinoEntry* e = wino_find(m, W, nmajor, tp);
  hipStream_t st = fwd_stream(m);
  if (!e) {
    DV_TRY(wino_register(m, W, nmajor, tp, Cin, Cout, &e));
    DV_TRY(wino_upload_descs(m, st));
  }
  // Staleness is dealt with at the head of a forward pass (wino_refresh_all), once for all layers.  Here only an entry
  // that has never been computed is transformed (a layer registered on the fly: the debug harness): the parameter epoch
  // also moves DURING a backward pass - the decoder bucket is updated on the comm stream while the encoder is still
  // being differentiated - and the data-gradient forms must keep the weights the forward pass used.
  if (e->epoch == ~(uint64_t)0) {
    const size_t i = (size_t)(e - m->wino.data());
    ProfScope ps(m, 2, st);
    DV_TRY(launch_wino_weights(m->wino_descs_dev + i, &e->d, 1, st));
    e->epoch = m->param_epoch;
  }
  WinoParams p;
  memset(&p, 0, sizeof p);
  p.X = X; p.Ut = e->d.Ut; p.U = U; p.A = Aout; p.bias = bias; p.alpha = alpha; p.zero = m->zero_page;
  p.NB = NB; p.H = H; p.Cin = Cin; p.Cout = Cout; p.epi = epi;
  // executed: groups of four 8 x 8-pixel blocks (16 tiles each) x 16 positions x Cin x Cout padded to 32-column tiles
  const double nbh = (H + 7) / 8, groups = ceil((double)NB * nbh * nbh / 4.0);
  const double exec = 2.0 * groups * 4.0 * 16.0 * 16.0 * (double)Cin * (double)(((Cout + 31) / 32) * 32);
  const double bytes = 4.0 * ((double)NB * H * H * (Cin + (U ? Cout : 0) + (Aout ? Cout : 0)) + 16.0 * Cin * Cout +
                              (epi == 2 ? (double)H * H * Cout : 0.0));
  ProfScope ps(m, 0, nullptr, PF_WINO, flops, exec, bytes);
  const int r = launch_wino_conv(p, st);
  if (r > 0) prof_uncount(m, 0, PF_WINO, flops, exec, bytes);
  return r;
}

// fprop-form gconv over an [NB,Hin,Hin,Cin] tensor: out[NB,Hout,Hout,Cout], in pixel = out*s + k - pb
// ksz: kernel size (model.py:81-91,121-134 take kernels[i] freely).  3 (and the one-tap dense form) have the specialised
// kernel families; every other size takes the general gather-GEMM (gconv.hip) with its tap table.
static int gconv_fprop(dv_model* m, const float* X, const float* W, bool nmajor, const float* bias, const float* alpha,
                       float* U, float* Aout, int epi, int NB, int Hin, int Cin, int Hout, int Cout, int s, int pb,
                       bool single_tap = false, const FuseBwd* fz = nullptr, bool* fused = nullptr, int ksz = 3) {
  if (fused) *fused = false;
  if (single_tap && Hin == 1 && exp_skip_dense()) return OK;
  GConvParams p;
  memset(&p, 0, sizeof p);
  p.X = X;
  p.W = W;
  p.U = U;
  p.A = Aout;
  p.bias = bias;
  p.alpha = alpha;
  p.NB = NB;
  p.Hin = p.Win = Hin;
  p.Cin = Cin;
  p.Hout = p.Wout = Hout;
  p.Cout = Cout;
  p.Hc = p.Wc = Hout;
  p.sin = s;
  p.sout = 1;
  p.ph = p.pw = 0;
  p.M = NB * Hout * Hout;
  p.w_nmajor = nmajor ? 1 : 0;
  p.epi = epi;
  Taps one;
  one.add(0, 0, 0);
  const Taps tp = single_tap ? one : taps_fprop(pb, ksz);
  const bool k3 = single_tap || ksz == 3;          // the specialised families speak the 3 x 3 tap code
  // algorithmic FLOPs of this launch (padding taps counted; the folded first conv and the padded head count their real channels)
  const double flops = 2.0 * NB * Hout * Hout * tp.n * (double)(W == m->W1p ? m->A.C : Cin) *
                       (double)(W == m->Whp ? 2 * m->A.C : Cout);
  if (k3 && s == 1 && pb == 1 && Hin == Hout && tp.n == 9 && !single_tap && !g_force_v1 && !g_no_special && !(fz && !m->no_fuse)) {
    const int r = wino_conv(m, X, W, nmajor, tp, bias, alpha, U, Aout, epi, NB, Hout, Cin, Cout, flops);
    if (r <= 0) return r;
  }
  if (k3 && Cin == 32 && (Cout == 16 || Cout == 32) && s == 1 && Hin == Hout && Hout >= 8 && Hout <= 64 && tp.n == 9 &&
      !single_tap && !g_force_v1 && !g_no_special && !(fz && !m->no_fuse)) {
    GStripParams g;
    memset(&g, 0, sizeof g);
    g.X = X; g.W = W; g.U = U; g.A = Aout; g.bias = bias; g.alpha = alpha; g.zero = m->zero_page;
    g.NB = NB; g.H = Hout; g.Wd = Hout; g.Cin = Cin; g.Cout = Cout;
    g.tapcode = tp.tapcode; g.wtcode = tp.wtcode; g.epi = epi;
    int r;
    {
      ProfScope ps(m, 0, nullptr, PF_GSTRIP, flops);
      r = launch_gconv_strip(g, nmajor, fwd_stream(m));
      if (r > 0) prof_uncount(m, 0, PF_GSTRIP, flops);
    }
    if (r <= 0) return r;
  }
  if (k3 && Cin == 8 && Cout == 32 && s == 1 && pb == 1 && !nmajor && Hin == Hout && Hout >= 8 && Hout <= 64 && tp.n == 9 &&
      !single_tap && !g_force_v1 && !g_no_special && !fz) {
    GStripParams g;                                  // first layer: strip form
    memset(&g, 0, sizeof g);
    g.X = X; g.W = W; g.U = U; g.A = Aout; g.bias = bias; g.alpha = alpha; g.zero = m->zero_page;
    g.NB = NB; g.H = Hout; g.Wd = Hout; g.Cin = Cin; g.Cout = Cout; g.epi = epi;
    int r;
    {
      ProfScope ps(m, 0, nullptr, PF_GSTRIP8, flops);
      r = launch_gconv_strip8(g, fwd_stream(m));
      if (r > 0) prof_uncount(m, 0, PF_GSTRIP8, flops);
    }
    if (r <= 0) return r;
  }
  if (single_tap && nmajor && Hin == 1 && Hout == 1 && Cout <= 64 && Cin <= 1024 && epi == 0 && !bias && !fz && !g_force_v1 &&
      !g_no_special) {
    // narrow dense data gradient (hidden -> latent_dim): one wave per stamp instead of two serial 128 x 32 tiles
    ProfScope ps(m, 2);                                // (9 MFLOP per step: timed with the small kernels, not as a matrix family)
    if (exp_skip_small()) return OK;
    return launch_dense_narrow(X, W, U, NB, Cin, Cout, fwd_stream(m));
  }
  // (dense operands whose width is a multiple of 4 but not of 32 - the 560-wide ones - take the ragged-K form of gconv2)
  const bool ragged_dense = single_tap && Cin > 32 && (Cin & 3) == 0 && (Cin % 32) != 0 && !fz && !g_no_special;
  if ((Cin % 32 == 0 || ragged_dense || ((Cin == 8 || Cin == 16) && Cout <= 32 && !single_tap)) && !g_force_v1 && k3 &&
      tp.legacy) {
    GConv2Params q;
    memset(&q, 0, sizeof q);
    q.X = X; q.W = W; q.U = U; q.A = Aout; q.bias = bias; q.alpha = alpha;
    q.NB = NB; q.Hin = q.Win = Hin; q.Cin = Cin; q.Hout = q.Wout = Hout; q.Cout = Cout;
    q.sin = s; q.sout = 1; q.nclass = 1;
    q.cls[0].Hc = q.cls[0].Wc = Hout; q.cls[0].M = NB * Hout * Hout; q.cls[0].ph = q.cls[0].pw = 0;
    q.cls[0].ntaps = tp.n; q.cls[0].tapcode = tp.tapcode; q.cls[0].wtcode = tp.wtcode;
    q.w_nmajor = nmajor ? 1 : 0; q.epi = epi;
    // dense-shaped contractions (few output tiles, long K): slice K over blockIdx.y into ws1 slabs
    const long MN = (long)NB * Hout * Hout * Cout;
    const long tiles64 = ((q.cls[0].M + 63) / 64) * (long)((Cout + 63) / 64);
    const int nchunks = tp.n * ((Cin + 31) / 32);
    if (single_tap && tiles64 < 256 && nchunks >= 32 && m->ws4) {
      const size_t ws4_cap = m->ws4_elems / 4;
      float* ws4 = m->ws4 + (size_t)m->lane_id * ws4_cap;   // each forward lane owns a quarter of the split-K workspace
      int ks = (int)std::min<long>(std::min<long>(16, nchunks / 8), (long)(ws4_cap / (size_t)MN));
      if (ks > 1) {
        q.ksplit = ks;
        q.U = ws4;
        q.A = nullptr;
        q.epi = 0;
        {
          ProfScope ps(m, 0, nullptr, PF_GCONV2, flops);
          DV_TRY(launch_gconv2(q, fwd_stream(m)));
        }
        ProfScope ps(m, 2);
        if (exp_skip_small()) return OK;
        return launch_splitk_finish(ws4, ks, MN, Cout, epi >= 1 ? bias : nullptr, epi == 2 ? alpha : nullptr,
                                    (long)Hout * Hout * Cout, U, epi == 2 ? Aout : nullptr, fwd_stream(m));
      }
    }
    if (!fz && !single_tap) {
      const int r = gconv2_small_splitk(m, q, NB, Hout, Cout, nchunks, epi, bias, alpha, U, Aout, flops);
      if (r != 0) return r < 0 ? r : OK;
    }
    long db_rows = 0;
    const bool fuse = fz && !m->no_fuse && fuse_setup(m, q, fz, &db_rows) == OK;
    {
      ProfScope ps(m, 0, nullptr, PF_GCONV2, flops);
      DV_TRY(launch_gconv2(q, fwd_stream(m)));
    }
    if (fuse) {
      if (fused) *fused = true;
      return fuse_finish(m, q, fz, db_rows);
    }
    return OK;
  }
  fill_gconv_common(p, tp, Cin);
  ProfScope ps(m, 0, nullptr, PF_GCONV, flops);
  return launch_gconv(p, fwd_stream(m));
}

// data-gradient-form gconv: target [NB,Ht,Ht,Ct] (s*s parity classes), source [NB,Hs,Hs,Cs];
// target pixel o satisfies o + pb = s*i + k for source pixel i.
static int gconv_dgrad(dv_model* m, const float* X, const float* W, bool nmajor, const float* bias, const float* alpha,
                       float* U, float* Aout, int epi, int NB, int Hs, int Cs, int Ht, int Ct, int s, int pb,
                       const FuseBwd* fz = nullptr, bool* fused = nullptr, int ksz = 3) {
  if (fused) *fused = false;
  // algorithmic FLOPs: every source pixel meets all k*k taps; the padded head gradient counts 2*bands channels
  const double flops = 2.0 * NB * Hs * Hs * (double)(ksz * ksz) * (double)(W == m->Whp ? 2 * m->A.C : Cs) * (double)Ct;
  const bool k3 = ksz == 3;
  if (k3 && s == 1 && pb == 1 && Hs == Ht && !g_force_v1 && !g_no_special && !(fz && !m->no_fuse)) {
    const Taps tp = taps_dgrad(1, pb, 0, 0);
    if (tp.n == 9) {
      const int r = wino_conv(m, X, W, nmajor, tp, bias, alpha, U, Aout, epi, NB, Ht, Cs, Ct, flops);
      if (r <= 0) return r;
    }
  }
  if (k3 && s == 1 && (Cs == 32 || (Cs == 16 && Ct == 32)) && (Ct == 16 || Ct == 32) && Hs == Ht && Ht >= 8 && Ht <= 64 && !g_force_v1 && !g_no_special &&
      !(fz && !m->no_fuse)) {
    const Taps tp = taps_dgrad(1, pb, 0, 0);
    if (tp.n == 9) {
      GStripParams g;
      memset(&g, 0, sizeof g);
      g.X = X; g.W = W; g.U = U; g.A = Aout; g.bias = bias; g.alpha = alpha; g.zero = m->zero_page;
      g.NB = NB; g.H = Ht; g.Wd = Ht; g.Cin = Cs; g.Cout = Ct;
      g.tapcode = tp.tapcode; g.wtcode = tp.wtcode; g.epi = epi;
      int r;
      {
        ProfScope ps(m, 0, nullptr, PF_GSTRIP, flops);
        r = launch_gconv_strip(g, nmajor, fwd_stream(m));
        if (r > 0) prof_uncount(m, 0, PF_GSTRIP, flops);
      }
      if (r <= 0) return r;
    }
  }
  // (tiny inference calls take the parity-class form below instead: it can slice K over workgroups, the fused kernel cannot)
  const bool tiny_splitk = m->tiny_call && NB <= 16 && !fz;
  if (k3 && s == 2 && Cs % 32 == 0 && Ct % 4 == 0 && nmajor && !g_force_v1 && !g_no_special && !(fz && !m->no_fuse) &&
      !tiny_splitk) {
    // all four parity classes in one workgroup (gconv_s2.hip)
    GConvS2Params q;
    memset(&q, 0, sizeof q);
    q.X = X; q.W = W; q.U = U; q.A = Aout; q.bias = bias; q.alpha = alpha;
    q.NB = NB; q.Hin = q.Win = Hs; q.Cin = Cs; q.Hout = q.Wout = Ht; q.Cout = Ct;
    q.Hc = q.Wc = (Ht + 1) / 2; q.M = NB * q.Hc * q.Wc; q.epi = epi;
    // per dimension: the parity with two kernel taps, its extra source offset x, and the kernel index per (parity, offset)
    int two = -1, x = 0, kk[2][2] = {{-1, -1}, {-1, -1}};
    bool ok = true;
    for (int ph = 0; ph < 2; ++ph) {
      int n = 0;
      for (int kh = 0; kh < 3; ++kh) {
        const int nh = ph + pb - kh;
        if (nh & 1) continue;
        const int d = nh / 2;
        ++n;
        if (d == 0) kk[ph][0] = kh; else { kk[ph][1] = kh; x = d; two = ph; }
      }
      if (kk[ph][0] < 0 || n > 2) ok = false;
    }
    if (ok && two >= 0 && kk[1 - two][1] < 0) {
      for (int c = 0; c < 4; ++c) {
        q.cph[c] = (c & 2) ? two : 1 - two;
        q.cpw[c] = (c & 1) ? two : 1 - two;
      }
      for (int e = 0; e < 4; ++e) {
        q.ndh[e] = (e & 2) ? x : 0;
        q.ndw[e] = (e & 1) ? x : 0;
        for (int c = 0; c < 4; ++c)
          if ((e & ~c) == 0) q.wt[e][c] = kk[q.cph[c]][(e & 2) ? 1 : 0] * 3 + kk[q.cpw[c]][(e & 1) ? 1 : 0];
      }
      ProfScope ps(m, 0, nullptr, PF_GCONV_S2, flops);
      return launch_gconv_s2(q, fwd_stream(m));
    }
  }
  if (k3 && (Cs % 32 == 0 || ((Cs == 8 || Cs == 16) && Ct <= 32)) && s <= 2 && !g_force_v1) {
    GConv2Params q;
    memset(&q, 0, sizeof q);
    q.X = X; q.W = W; q.U = U; q.A = Aout; q.bias = bias; q.alpha = alpha;
    q.NB = NB; q.Hin = q.Win = Hs; q.Cin = Cs; q.Hout = q.Wout = Ht; q.Cout = Ct;
    q.sin = 1; q.sout = s; q.w_nmajor = nmajor ? 1 : 0; q.epi = epi;
    // heaviest parity class first so the short ones fill the tail of the launch
    struct C { int ph, pw, n; } order[4];
    int nc = 0;
    for (int ph = 0; ph < s; ++ph)
      for (int pw = 0; pw < s; ++pw) order[nc++] = {ph, pw, taps_dgrad(s, pb, ph, pw).n};
    std::sort(order, order + nc, [](const C& a, const C& b) { return a.n > b.n; });
    int k = 0;
    for (int i = 0; i < nc; ++i) {
      int hc = (Ht - order[i].ph + s - 1) / s, wc = (Ht - order[i].pw + s - 1) / s;
      if (hc <= 0 || wc <= 0) continue;
      Taps t = taps_dgrad(s, pb, order[i].ph, order[i].pw);
      if (t.n == 0) {
        set_error("empty parity class");
        return E_INVALID;
      }
      GClass2& c = q.cls[k++];
      c.Hc = hc; c.Wc = wc; c.M = NB * hc * wc; c.ph = order[i].ph; c.pw = order[i].pw;
      c.ntaps = t.n; c.tapcode = t.tapcode; c.wtcode = t.wtcode;
    }
    q.nclass = k;
    if (!fz && k >= 1 && Cs % 32 == 0) {
      int maxtaps = 0;                                 // (classes with fewer chunks write zero slabs for the rest)
      for (int i = 0; i < k; ++i) maxtaps = std::max(maxtaps, q.cls[i].ntaps);
      const int r = gconv2_small_splitk(m, q, NB, Ht, Ct, maxtaps * (Cs / 32), epi, bias, alpha, U, Aout, flops);
      if (r != 0) return r < 0 ? r : OK;
    }
    long db_rows = 0;
    const bool fuse = fz && !m->no_fuse && fuse_setup(m, q, fz, &db_rows) == OK;
    {
      ProfScope ps(m, 0, nullptr, PF_GCONV2, flops);
      DV_TRY(launch_gconv2(q, fwd_stream(m)));
    }
    if (fuse) {
      if (fused) *fused = true;
      return fuse_finish(m, q, fz, db_rows);
    }
    return OK;
  }
  for (int ph = 0; ph < s; ++ph)
    for (int pw = 0; pw < s; ++pw) {
      int hc = (Ht - ph + s - 1) / s, wc = (Ht - pw + s - 1) / s;
      if (hc <= 0 || wc <= 0) continue;
      Taps t = taps_dgrad(s, pb, ph, pw, ksz);
      GConvParams p;
      memset(&p, 0, sizeof p);
      p.X = X;
      p.W = W;
      p.U = U;
      p.A = Aout;
      p.bias = bias;
      p.alpha = alpha;
      p.NB = NB;
      p.Hin = p.Win = Hs;
      p.Cin = Cs;
      p.Hout = p.Wout = Ht;
      p.Cout = Ct;
      p.Hc = hc;
      p.Wc = wc;
      p.sin = 1;
      p.sout = s;
      p.ph = ph;
      p.pw = pw;
      p.M = NB * hc * wc;
      p.w_nmajor = nmajor ? 1 : 0;
      p.epi = epi;
      // (a class without taps - odd output pixels of a 1x1 stride-2 Conv2DTranspose - is legal: its pixels receive the
      // bias alone, or a zero gradient; the kernel then runs its epilogue on zero accumulators)
      fill_gconv_common(p, t, Cs);
      ProfScope ps(m, 0, nullptr, PF_GCONV, flops * t.n / (double)(ksz * ksz));
      DV_TRY(launch_gconv(p, fwd_stream(m)));
    }
  return OK;
}

// dW = sum_p Xg[p,t][cx] * Y[p][cy]; X pixel = grid*sx + k - pb; result rows (wt,cx) x cols cy into `out`
static int wgrad_impl(dv_model* m, hipStream_t ws, const float* X, int Hx, int Cx, const float* Y, int Hy, int Cy, int NB,
                      int sx, int pb, bool single_tap, float* out, int cpad, int creal, const FuseBwd* fz, int ksz);

// Weight gradients are queued on m->wstream.  When that is the aux stream, the call first makes it wait for
// everything the main stream has produced so far (the operand d(pre-activation) is final at this point).
// on_main: queue this launch (and its slab reduction) on the main stream even when the weight gradients run on the
// aux stream - used for the last one of the step, when the main stream has nothing else left to do.
static int wgrad(dv_model* m, const float* X, int Hx, int Cx, const float* Y, int Hy, int Cy, int NB, int sx, int pb,
                 bool single_tap, float* out, int cpad, int creal, const FuseBwd* fz = nullptr, bool on_main = false,
                 int ksz = 3) {
  hipStream_t ws = (m->wstream && !on_main) ? m->wstream : m->ctx->stream;
  if (ws != m->ctx->stream) {
    // the PReLU backward just queued may already have recorded the main stream's position (for its reductions)
    if (!m->main_marked) DV_HIP(hipEventRecord(m->ctx->ev_ready, m->ctx->stream));
    DV_HIP(hipStreamWaitEvent(ws, m->ctx->ev_ready, 0));
  }
  m->main_marked = false;
  return wgrad_impl(m, ws, X, Hx, Cx, Y, Hy, Cy, NB, sx, pb, single_tap, out, cpad, creal, fz, ksz);
}

// fz (first layer only, Cx == 8): Y is d(activation); the strip kernel applies the PReLU backward of fz on the fly
// and also produces d(alpha) / d(bias), see wgrad_strip8_kernel<true>.
static int wgrad_impl(dv_model* m, hipStream_t ws, const float* X, int Hx, int Cx, const float* Y, int Hy, int Cy, int NB,
                      int sx, int pb, bool single_tap, float* out, int cpad, int creal, const FuseBwd* fz, int ksz) {
  const bool k3 = ksz == 3;
  {   // DV_EXP_SKIP_WGRAD=2 (MEASUREMENT, wrong gradients): no conv weight-gradient work at all (all three families and their
      // slab sums; the fused first layer and the dense layers stay) - what the whole weight-gradient stream costs the step
    static const int exp_all = DV_EXP_SWITCH("DV_EXP_SKIP_WGRAD");
    if (exp_all == 2 && !single_tap && !fz) return OK;
    if (single_tap && exp_skip_dense()) return OK;
  }
  // slab region and the stream that sums the slabs: with the weight gradients on the aux stream the reduction goes to
  // the reduction stream and the slabs rotate through three regions of ws1
  dv_ctx* cx = m->ctx;
  const double wflops = 2.0 * NB * Hy * Hy * (single_tap ? 1.0 : (double)(ksz * ksz)) * (double)(X == m->xn ? m->A.C : Cx) *
                        (double)(out == m->Ghs ? 2 * m->A.C : Cy);
  {
    // Dense layers (one tap, one pixel: out[cx][cy] = sum over stamps): a stamp-major one-pass kernel that writes the
    // gradient itself - no slab region, no slab sum - exists (dense_wgrad_tn_kernel, round 6), is parity-green, and is NOT
    // the default: in the overlapped step it is slower than the tiled kernel + slab sum it would replace (fp32 4.594 ->
    // 4.630 ms, bf16 1.882 -> 1.910 ms, alternating runs, profiles/r06_exp_dense_wgrad_onepass.txt): 576 - 1152 waves that
    // each walk all 256 stamps as one dependent chain hold their CUs longer than 160 short-K tiles do.  Opt-in for the A/B.
    static const bool onepass = getenv("DV_DENSE_WGRAD_ONEPASS") != nullptr;
    if (single_tap && Hx == 1 && Hy == 1 && sx == 1 && cpad == creal && !fz && !g_force_v1 && !g_no_special && onepass &&
        !(Cx & 1) && !(Cy & 3)) {
      {
        ProfScope ps(m, 1, ws, PF_WGRAD, wflops);
        DV_TRY(launch_dense_wgrad_tn(X, Cx, Y, Cy, NB, Cx, Cy, out, Cy, ws));
      }
      m->ws_last_rs = ws;
      m->ws_last = -1;
      return OK;
    }
  }
  // the regions rotate whenever weight-gradient work may be in flight on the aux stream, also for a launch that is
  // itself queued on the main stream (which then reduces its own slabs: no stream hop)
  const bool rot = m->wstream && m->wstream != cx->stream && m->arena_reduce && cx->red_stream && m->ev_wk[0];
  const bool per_launch = m->ws_nreg > 3;      // one region per launch of the step: nothing to wait for
  float* part = m->ws1;
  size_t part_cap = m->ws1_elems;
  hipStream_t rs = ws;
  int reg = -1;
  if (rot) {
    if (per_launch) {
      if (m->ws_count >= m->ws_nreg) {
        set_error("more weight-gradient launches in a step than slab regions (%d)", m->ws_nreg);
        return E_STATE;
      }
      reg = m->ws_count++;
      part_cap = m->ws_region_cap;
      part = m->ws1x + (size_t)reg * part_cap;
    } else {
      reg = m->ws_region;
      m->ws_region = (reg + 1) % 3;
      part_cap = m->ws1_elems / 3;
      part = m->ws1 + (size_t)reg * part_cap;
      if (m->ws_pending[reg]) {          // the reduction that last read this region must be done before it is rewritten
        DV_HIP(hipStreamWaitEvent(ws, m->ev_rk[reg], 0));
        m->ws_pending[reg] = false;
      }
    }
    if (ws != cx->stream) rs = cx->red_stream;
  }
  auto hand_over = [&]() -> int {        // slabs written on ws -> reduction on rs
    if (!rot || rs == ws) return OK;
    DV_HIP(hipEventRecord(m->ev_wk[reg % 3], ws));
    DV_HIP(hipStreamWaitEvent(rs, m->ev_wk[reg % 3], 0));
    return OK;
  };
  auto reduced = [&]() -> int {
    if (!rot) return OK;
    m->ws_last_rs = rs;
    if (per_launch) return OK;           // wgrad_result_ready records on demand
    DV_HIP(hipEventRecord(m->ev_rk[reg], rs));
    m->ws_pending[reg] = true;
    m->ws_last = reg;
    return OK;
  };
  if (k3 && !single_tap && sx == 1 && pb == 1 && Hx == Hy && cpad == creal && !fz && !g_force_v1 && !g_no_special && !g_no_wino &&
      m->use_wino && !m->bf.on && m->zero_page && wino_wgrad_supported(NB, Hy, Cx, Cy)) {
    // stride-1 layers with >= 64 channels on both sides: Winograd-domain weight gradient (wino.hip), its partial slabs in
    // a buffer of this launch's own (allocated at first use: 64 MiB per launch at 256 CUs)
    int S = 1;
    const size_t need = wino_wgrad_part_floats(NB, Hy, Cx, Cy, &S);
    const int wi = m->wino_wcount++;
    if ((int)m->wino_wslabs.size() <= wi) m->wino_wslabs.resize(wi + 1, {nullptr, 0});
    if (m->wino_wslabs[wi].second < need) {
      float* q = nullptr;
      if (hipMalloc((void**)&q, need * sizeof(float)) == hipSuccess) {
        m->allocs.push_back(q);
        m->wino_wslabs[wi] = {q, need};            // (a smaller predecessor stays in allocs until the model goes)
      } else {
        (void)hipGetLastError();
      }
    }
    if (m->wino_wslabs[wi].second >= need) {
      WinoWgradParams wp;
      memset(&wp, 0, sizeof wp);
      wp.X = X; wp.Y = Y; wp.part = m->wino_wslabs[wi].first; wp.part_capacity = m->wino_wslabs[wi].second;
      wp.zero = m->zero_page; wp.NB = NB; wp.H = Hy; wp.Cx = Cx; wp.Cy = Cy;
      int st;
      {
        const double nbh = (Hy + 7) / 8;
        const double exec = 2.0 * (double)NB * nbh * nbh * 16.0 * 16.0 * (double)Cx * (double)Cy;
        const double bytes = 4.0 * ((double)NB * Hy * Hy * (Cx + Cy) + (double)S * 16.0 * Cx * Cy);
        ProfScope ps(m, 1, ws, PF_WINOW, wflops, exec, bytes);
        static const bool exp_skip_winow = DV_EXP_SWITCH("DV_EXP_SKIP_WGRAD") == 3;   // (3: the Winograd-domain launches only)
        st = exp_skip_winow ? OK : launch_wino_wgrad(wp, out, ws);
        if (st > 0) prof_uncount(m, 1, PF_WINOW, wflops, exec, bytes);
      }
      if (st < 0) return st;
      if (st == 0) {
        DV_TRY(hand_over());
        {
          ProfScope ps(m, 2, rs);
          DV_TRY(launch_wino_wgrad_finish(wp.part, out, S, Cx, Cy, rs));
        }
        return reduced();
      }
    }
  }
  if (k3 && !single_tap && !g_force_v1 && !(g_no_special && !fz) && cpad == creal && wgrad_strip_supported(Cx, Cy, sx, 9)) {
    WStripParams sp;
    memset(&sp, 0, sizeof sp);
    sp.X = X; sp.Y = Y; sp.part = part; sp.part_capacity = part_cap;
    sp.NB = NB; sp.Hx = sp.Wx = Hx; sp.Hy = sp.Wy = Hy; sp.pb = pb;
    sp.zero = m->zero_page;
    int ns = 0, st, groups = 0;
    if (fz) {
      // partial sums of d(alpha) ([groups][E]) and d(bias) ([workgroups][Cy]): from the per-step arena when another
      // stream reduces them, else from ws2 / ws3
      const Arch& A = m->A;
      const long E = (long)Hy * Hy * Cy;
      const bool arena = rs != ws;
      const size_t dbcap = (size_t)1024 * Cy;
      if (arena) {
        if (m->arena_off + (size_t)E + dbcap > m->arena_elems) {
          set_error("gradient-partial arena exhausted");
          return E_STATE;
        }
        sp.db_part = m->arena + m->arena_off;
        m->arena_off += dbcap;
        sp.dal_part = m->arena + m->arena_off;
        sp.dal_capacity = std::min(m->arena_elems - m->arena_off, (size_t)32 * E);
        m->arena_off += sp.dal_capacity;
      } else {
        if (dbcap > m->ws3_elems) {
          set_error("bias-gradient workspace too small");
          return E_STATE;
        }
        sp.db_part = m->ws3;
        sp.dal_part = m->ws2;
        sp.dal_capacity = m->ws2_elems;
      }
      sp.db_capacity = dbcap;
      sp.U = fz->u;
      sp.alpha = fz->alpha_ptr ? fz->alpha_ptr : m->P + A.specs[fz->alpha_spec].off;
      sp.alpha_elems = E;
      sp.groups_out = &groups;
    }
    {
      ProfScope ps(m, 1, ws, PF_WSTRIP, wflops);
      static const bool exp_skip_strip = DV_EXP_SWITCH("DV_EXP_SKIP_WGRAD") == 4;     // (4: the strip launches only, not the fused first layer)
      if (exp_skip_strip && !fz) {
        st = OK;
        ns = (int)std::min<size_t>(256, part_cap / ((size_t)9 * Cx * Cy));             // (the slabs it would have written)
      } else {
        st = launch_wgrad_strip(sp, Cx, Cy, sx, ws, &ns);
      }
      if (st > 0) prof_uncount(m, 1, PF_WSTRIP, wflops);
    }
    if (st < 0) return st;
    if (st > 0 && fz) {
      set_error("fused first-layer weight gradient: geometry not supported");
      return E_STATE;
    }
    if (st == 0) {
      DV_TRY(hand_over());
      {
        ProfScope ps(m, 2, rs);
        DV_TRY(launch_reduce_partials(part, out, ns, (long)9 * Cx * Cy, Cy, cpad, creal, rs));
        if (fz) {
          const Arch& A = m->A;
          float* dal_out = fz->dalpha_out ? fz->dalpha_out : m->G + A.specs[fz->alpha_spec].off;
          float* db_out = fz->dbias_out ? fz->dbias_out : m->G + A.specs[fz->bias_spec].off;
          DV_TRY(launch_reduce_partials(sp.dal_part, dal_out, groups, sp.alpha_elems, 4, 1, 1, rs));
          DV_TRY(launch_reduce_rows_f64(sp.db_part, ns, Cy, db_out, 1.0f, rs));
        }
      }
      return reduced();
    }
    // st > 0: the strip form does not fit this geometry (very wide rows): use the tiled kernel below
  }
  WGradParams p;
  memset(&p, 0, sizeof p);
  Taps t;
  if (single_tap)
    t.add(0, 0, 0);
  else
    t = taps_fprop(pb, ksz);
  if (fz) {
    set_error("the fused first-layer weight gradient exists for 3x3 kernels only");
    return E_STATE;
  }
  p.X = X;
  p.Y = Y;
  p.part = part;
  p.NB = NB;
  p.Hx = p.Wx = Hx;
  p.Cx = Cx;
  p.Hy = p.Wy = Hy;
  p.Cy = Cy;
  p.Hc = p.Wc = Hy;
  p.sx = sx;
  p.sy = 1;
  p.ph = p.pw = 0;
  p.ntaps = t.n;
  p.xt = t.xt;
  p.P = NB * Hy * Hy;
  p.rows_total = t.n * Cx;
  long slab = (long)p.rows_total * Cy;
  long tiles = ((p.rows_total + 127) / 128) * (long)((Cy + 127) / 128);
  // At most one round of resident workgroups (two 74 KB workgroups per CU x 256 CUs), never a round and a half: alone, 540
  // workgroups run as long as 1024 and 504 finish 8 % sooner (tools/layer_bench.py).  In the overlapped step - the kernel
  // shares the chip with the main stream's persistent one-workgroup-per-CU Winograd launches - fewer, longer pixel ranges
  // do better still: 384 gives 4.74 ms per step against 4.83 with 512 and 4.80 with 256 (same box, alternating runs)
  const long target = 384;
  long ns = std::max(1L, target / tiles);
  ns = std::min(ns, (long)std::max(1, p.P / 256));
  ns = std::min(ns, 256L);
  ns = std::min(ns, (long)(part_cap / (size_t)slab));
  ns = std::max(ns, 1L);
  if ((size_t)slab > part_cap) {
    set_error("wgrad workspace too small");
    return E_STATE;
  }
  int pchunk = (int)((p.P + ns - 1) / ns);
  pchunk = (pchunk + 31) & ~31;
  ns = (p.P + pchunk - 1) / pchunk;
  p.nsplit = (int)ns;
  p.pchunk = pchunk;
  // DV_EXP_SKIP_WGRAD=1 (a MEASUREMENT switch, gradients are wrong): the tiled weight-gradient launches of the conv layers
  // are left out, slab sums and stream hand-overs kept - the upper bound of what a faster wgrad_kernel can give the step
  static const bool exp_skip = DV_EXP_SWITCH("DV_EXP_SKIP_WGRAD") == 1 || DV_EXP_SWITCH("DV_EXP_SKIP_WGRAD") == 2;
  if (!(exp_skip && !single_tap)) {
    ProfScope ps(m, 1, ws, PF_WGRAD, wflops);
    DV_TRY(launch_wgrad(p, ws));
  }
  DV_TRY(hand_over());
  {
    ProfScope ps(m, 2, rs);
    DV_TRY(launch_reduce_partials(part, out, p.nsplit, slab, Cy, cpad, creal, rs));
  }
  return reduced();
}

// makes `ws` wait for the reduction that produced the most recent weight gradient (its consumer runs on ws)
// makes stream ws wait for the slab reduction of the weight gradient queued last
static int wgrad_result_ready(dv_model* m, hipStream_t ws) {
  if (m->ws_nreg > 3) {
    if (m->ws_last_rs && m->ws_last_rs != ws) {
      DV_HIP(hipEventRecord(m->ev_rk[0], m->ws_last_rs));
      DV_HIP(hipStreamWaitEvent(ws, m->ev_rk[0], 0));
    }
    return OK;
  }
  if (m->ws_last >= 0 && m->ws_pending[m->ws_last]) DV_HIP(hipStreamWaitEvent(ws, m->ev_rk[m->ws_last], 0));
  return OK;
}

// Allocates the per-step buffer pool of the "no reuse" mode (once; on failure the rotating forms stay in use).
static void ensure_step_pool(dv_model* m) {
  if (m->step_pool_tried) return;
  m->step_pool_tried = true;
  const Arch& A = m->A;
  const int nbuf = 4 * A.L + 10, nreg = 4 * A.L + 8;
  const size_t cap = m->ws1_elems / 3;
  float *pool = nullptr, *slabs = nullptr;
  if (hipMalloc((void**)&pool, (size_t)(nbuf - 3) * m->max_act_elems * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  if (hipMalloc((void**)&slabs, (size_t)nreg * cap * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(pool);
    return;
  }
  m->allocs.push_back(pool);
  m->allocs.push_back(slabs);
  m->gpool = pool;
  for (int k = 0; k < nbuf - 3; ++k) m->gbufs.push_back(pool + (size_t)k * m->max_act_elems);
  m->ws1x = slabs;
  m->ws_region_cap = cap;
  m->ws_nreg = nreg;
}

// PReLU backward with optional parameter gradients.  du is needed by the next launches of the main stream; the
// reductions that turn the d(alpha) / d(bias) partials into gradients are not, so (when the aux stream is in use)
// they are queued there, reading partials from a per-step bump arena that no later main-stream kernel overwrites.
static int prelu_bwd(dv_model* m, float* da, const float* u, int alpha_spec, int bias_spec, int NB, int E, int C,
                     bool want_grads) {
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  // where the reductions go: a stream of their own, so that ~40 five-microsecond launches per step do not sit between
  // the weight-gradient kernels of the aux stream
  hipStream_t rs = (m->arena_reduce && m->wstream && m->wstream != s) ? m->ctx->red_stream : s;
  int gx = (E + 1023) / 1024;
  int nsplit = std::max(1, std::min(std::min(NB, 32), 1024 / std::max(gx, 1)));
  float *dal = nullptr, *dbp = nullptr;
  if (want_grads) {
    const bool arena = rs != s;
    size_t cap2 = arena ? m->arena_elems - m->arena_off : m->ws2_elems;
    size_t need3 = bias_spec >= 0 ? ((E == C) ? (size_t)nsplit * E : (size_t)nsplit * gx * C) : 0;
    need3 = (need3 + 3) & ~(size_t)3;
    while ((size_t)nsplit * E + need3 > cap2 && nsplit > 1) {
      --nsplit;
      need3 = bias_spec >= 0 ? ((E == C) ? (size_t)nsplit * E : (size_t)nsplit * gx * C) : 0;
      need3 = (need3 + 3) & ~(size_t)3;
    }
    if (arena) {
      if ((size_t)nsplit * E + need3 > cap2) {
        set_error("gradient-partial arena exhausted");
        return E_STATE;
      }
      dal = m->arena + m->arena_off;
      m->arena_off += (size_t)nsplit * E;
      if (bias_spec >= 0) {
        dbp = m->arena + m->arena_off;
        m->arena_off += need3;
      }
    } else {
      dal = m->ws2;
      if (bias_spec >= 0) {
        if (need3 > m->ws3_elems) {
          set_error("bias-gradient workspace too small");
          return E_STATE;
        }
        dbp = m->ws3;
      }
    }
  }
  int rows = 0;
  {
    ProfScope ps(m, 2);
    DV_TRY(launch_prelu_bwd(da, u, m->P + A.specs[alpha_spec].off, NB, E, C, nsplit, dal, dbp, &rows, s));
  }
  m->main_marked = false;
  if (want_grads) {
    if (rs != s) {
      DV_HIP(hipEventRecord(m->ctx->ev_ready, s));
      DV_HIP(hipStreamWaitEvent(rs, m->ctx->ev_ready, 0));
      m->main_marked = true;           // a weight-gradient launch queued next can wait on the same record
    }
    ProfScope ps(m, 2, rs);
    DV_TRY(launch_reduce_partials(dal, m->G + A.specs[alpha_spec].off, nsplit, E, 4, 1, 1, rs));
    if (dbp) DV_TRY(launch_reduce_rows_f64(dbp, rows, C, m->G + A.specs[bias_spec].off, 1.0f, rs));
  }
  return OK;
}

static int bias_grad_colsum(dv_model* m, const float* dy, long rows, int C, int ncols_out, int bias_spec) {
  int nr = 0;
  if ((size_t)(std::max<long>((rows + 2047) / 2048, 64) + 1) * C > m->ws3_elems) {
    set_error("colsum workspace too small");
    return E_STATE;
  }
  ProfScope ps(m, 2);
  if (exp_skip_small()) return OK;
  DV_TRY(launch_colsum(dy, rows, C, m->ws3, &nr, m->ctx->stream));
  return launch_reduce_rows_f64(m->ws3, nr, ncols_out, m->G + m->A.specs[bias_spec].off, 1.0f, m->ctx->stream, C);
}

// the operands the dense trunk reads (the parameters themselves unless the latent sizes needed padding)
static const float* enc_dense_w(const dv_model* m) { return m->Wdp ? m->Wdp : m->P + m->A.specs[m->A.enc_dk()].off; }
static const float* enc_dense_b(const dv_model* m) { return m->bdp ? m->bdp : m->P + m->A.specs[m->A.enc_db()].off; }
static float* enc_dense_g(dv_model* m) { return m->Gdp ? m->Gdp : m->G + m->A.specs[m->A.enc_dk()].off; }
static const float* dec_dense0_w(const dv_model* m) { return m->W0p ? m->W0p : m->P + m->A.specs[m->A.D0 + 1].off; }
static float* dec_dense0_g(dv_model* m) { return m->G0p ? m->G0p : m->G + m->A.specs[m->A.D0 + 1].off; }
// the gradient a padded weight-gradient launch left in its scratch -> the parameter's gradient, on the weight-gradient
// stream behind the launch's slab sum
static int wgrad_result_ready(dv_model* m, hipStream_t ws);
static int take_padded_grad(dv_model* m, const float* scratch, float* dst, int rows, int nsrc, int ndst) {
  hipStream_t ws = m->wstream ? m->wstream : m->ctx->stream;
  DV_TRY(wgrad_result_ready(m, ws));
  ProfScope ps(m, 2, ws);
  return launch_take_cols(scratch, dst, rows, nsrc, ndst, ws);
}
// rows of `width` floats between buffers whose row strides may differ (the padded latent tensors <-> the caller's dense arrays)
static int copy_rows(float* dst, size_t dst_ld, const float* src, size_t src_ld, size_t width, size_t rows, hipMemcpyKind kind,
                     hipStream_t s) {
  if (rows == 0) return OK;
  if (dst_ld == width && src_ld == width)
    DV_HIP(hipMemcpyAsync(dst, src, rows * width * sizeof(float), kind, s));
  else
    DV_HIP(hipMemcpy2DAsync(dst, dst_ld * sizeof(float), src, src_ld * sizeof(float), width * sizeof(float), rows, kind, s));
  return OK;
}

static int refresh_head_pad(dv_model* m, hipStream_t st = nullptr) {
  const Arch& A = m->A;
  m->bf.dirty_mask = 7;
  m->param_epoch++;
  if (!st) st = m->ctx->stream;
  if (m->W0p)      // decoder Dense 0 [d, hidden] -> [dp, hidden]: as one row of d * hidden floats padded to dp * hidden
    DV_TRY(launch_pad_cols(m->P + A.specs[A.D0 + 1].off, m->W0p, 1, A.d * A.dec_hidden, A.dp * A.dec_hidden, st));
  DV_TRY(launch_pad_cols(m->P + A.specs[A.head_k()].off, m->Whp, 9 * A.cfg.filters[0], 2 * A.C, A.C2p, st));
  return launch_pad_cols(m->P + A.specs[A.head_b()].off, m->bhp, 1, 2 * A.C, A.C2p, st);
}

static int refresh_w1p(dv_model* m) {
  const Arch& A = m->A;
  m->bf.dirty_mask = 7;
  m->param_epoch++;
  if (m->Wdp) {
    DV_TRY(launch_pad_cols(m->P + A.specs[A.enc_dk()].off, m->Wdp, A.flat, A.tw, A.twp, m->ctx->stream));
    DV_TRY(launch_pad_cols(m->P + A.specs[A.enc_db()].off, m->bdp, 1, A.tw, A.twp, m->ctx->stream));
  }
  return launch_pad_w1(m->P + A.specs[A.enc_k(0)].off, m->P + A.specs[0].off, m->P + A.specs[1].off, m->W1p,
                       A.enc_ksz(0) * A.enc_ksz(0), A.C, A.C0p, A.cfg.filters[0], m->ctx->stream);
}

// ---- forward ----------------------------------------------------------------------------------
// All forward helpers work on the lane [m->b0, m->b0 + NB) of the batch and queue on fwd_stream(m); with b0 = 0 and
// cs = null they are the plain whole-batch forms.
#define LANE(ptr, per_stamp) ((ptr) + (size_t)m->b0 * (size_t)(per_stamp))

// global batch statistics of the input BatchNorm (whole batch, main stream) -> m->bnstate
static int bn_prepare(dv_model* m, const float* xsrc, const int* idx, int first, int NB, int Bg, bool training,
                      bool upd_moving) {
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  const int HW = A.H * A.H;
  float* P = m->P;
  const float* sums = m->bnsums;
  if (training) {
    if (m->bn_pre_valid && idx == m->bn_pre_idx && xsrc == m->bn_pre_x && first == m->bn_pre_first &&
        NB == m->bn_pre_B && !m->prof_on) {
      // the batch sums (they depend on the data only) were computed and all-reduced on the comm stream during the
      // previous step: no reduction kernels and no latency-bound collective at the head of this step
      DV_TRY(main_waits_for_comm(m->ctx, m->ev_bnpre));
      sums = m->bn_pre_sums;
      if (m->bf.in_pre) {
        // bf16 engine: the prefetch also ran bn_finalize (moving statistics included) and the input kernel for this
        // batch on the comm stream: nothing left to do here
        if (!upd_moving) {
          set_error("a prefetched training input met a step that does not update the moving statistics");
          return E_STATE;
        }
        m->bn_pre_valid = false;
        m->bnpre_go_pending = true;
        return OK;
      }
    } else {
      if (m->bf.in_pre) {
        set_error("the input prefetched for the next training step does not match the step that follows");
        return E_STATE;
      }
      int nblk = 0;
      ProfScope ps(m, 2, s);
      // one 16-float partial row per 1024 pixels (pointwise.hip BN_PIX_PER_BLOCK): checked BEFORE the launch writes them
      if (((size_t)NB * HW + 1023) / 1024 * (2 * DV_BN_MAXC) > m->ws3_elems) {
        set_error("BN statistics workspace too small for %d stamps", NB);
        return E_STATE;
      }
      DV_TRY(launch_bn_stats(xsrc, idx, first, NB, HW, A.C, m->ws3, &nblk, s));
      DV_TRY(launch_reduce_rows_f64(m->ws3, nblk, 2 * DV_BN_MAXC, m->bnsums, 1.0f, s));
      DV_TRY(allreduce_small(m->ctx, m->bnsums, 2 * DV_BN_MAXC));
    }
    m->bn_pre_valid = false;
  }
  static int exp_calls = 0;
  if (!((exp_skip_tail() & 4) && ++exp_calls > 3)) {
    ProfScope ps(m, 2, s);
    DV_TRY(launch_bn_finalize(sums, (float)((double)Bg * HW), A.C, P + A.specs[0].off, P + A.specs[1].off,
                              P + A.specs[2].off, P + A.specs[3].off, A.cfg.bn_eps, A.cfg.bn_momentum,
                              A.cfg.bn_moving_var_unbiased, training ? 1 : 0, upd_moving ? 1 : 0, m->bnstate, s));
  }
  // the prefetched sums have been consumed: the comm stream may compute the next batch's into the same buffer (the bf16
  // engine records this behind its input kernel instead, bf_encoder_forward: bnstate and the input buffers are part of
  // what the next prefetch overwrites)
  if (sums == m->bn_pre_sums) {
    if (m->bf.on) m->bnpre_go_pending = true;
    else DV_HIP(hipEventRecord(m->ev_bnpre_go, s));
  }
  return OK;
}

static int bf_encoder_forward(dv_model* m, const float* xsrc, const int* idx, int first, int NB, bool keep_u, bool defer_t);
static int bf_decoder_forward(dv_model* m, int NB, bool keep_u);
static int bf_head_lane(dv_model* m, const float* ysrc, const int* idx, int first, int NB, int Bg, bool want_grad,
                        bool want_out, int part_block0, int* nblk);
static int bf_backward(dv_model* m, int NB, int Bg);
static int bf_flush_wred(dv_model* m, hipStream_t rs);
static void bf_head_fuse_request(dv_model* m, const float* ysrc, const int* idx, int first, int NB, int Bg, bool want_grad,
                                 bool want_out, int part_block0);

// encoder: dataset rows (idx / first) of the lane -> t
struct TinyCall {          // scope of one public inference call of at most 16 stamps
  dv_model* m;
  TinyCall(dv_model* mm, int64_t N) : m(mm) { m->tiny_call = N <= 16; }
  ~TinyCall() { m->tiny_call = false; }
};

struct LongCallKernels {   // scope inside a TinyCall in which kernels are selected as in a call of more than 16 stamps
  dv_model* m;
  bool was_tiny;
  explicit LongCallKernels(dv_model* mm) : m(mm), was_tiny(mm->tiny_call) { m->tiny_call = false; }
  ~LongCallKernels() { m->tiny_call = was_tiny; }
};

// DV_EXP_NO_A=<min size> (a MEASUREMENT switch, results are wrong): training forwards of the layers at least that many
// pixels wide store the pre-activation only (epilogue 1: no PReLU, no activation store) - the upper bound of what "store u
// only"  can save before any consumer pays for applying PReLU on load
static int exp_epi(bool keep_u, int hout) {
  static const int min_h = DV_EXP_SWITCH("DV_EXP_NO_A");
  return (min_h > 0 && keep_u && hout >= min_h) ? 1 : 2;
}

// defer_t: the caller runs sampler_forward right behind this call, which may then finish a K-split encoder Dense itself
static int encoder_forward(dv_model* m, const float* xsrc, const int* idx, int first, int NB, bool keep_u, bool defer_t = false) {
  if (m->bf.on) return bf_encoder_forward(m, xsrc, idx, first, NB, keep_u, defer_t);
  const Arch& A = m->A;
  hipStream_t s = fwd_stream(m);
  const int HW = A.H * A.H;
  float* P = m->P;
  float* xn = LANE(m->xn, (size_t)HW * A.C0p);
  static int exp_calls = 0;
  if (!((exp_skip_tail() & 4) && ++exp_calls > 3)) {
    ProfScope ps(m, 2);
    DV_TRY(launch_bn_apply(xsrc, idx ? idx + m->b0 : nullptr, first + m->b0, NB, HW, A.C, A.C0p, m->bnstate, xn, s));
  }
  const float* in = xn;
  for (int j = 0; j < 2 * A.L; ++j) {
    int hin, cin, hout, cout, st;
    A.enc_layer(j, &hin, &cin, &hout, &cout, &st);
    const int ksz = A.enc_ksz(j);
    int pb = same_pad_before(hin, ksz, st, nullptr);
    const float* W = j == 0 ? m->W1p : P + A.specs[A.enc_k(j)].off;
    int cin_phys = j == 0 ? A.C0p : cin;
    const size_t e_out = (size_t)hout * hout * cout;
    DV_TRY(gconv_fprop(m, in, W, false, P + A.specs[A.enc_b(j)].off, P + A.specs[A.enc_al(j)].off,
                       keep_u ? LANE(m->enc_u[j], e_out) : nullptr, LANE(m->enc_a[j], e_out), exp_epi(keep_u, hout), NB, hin,
                       cin_phys, hout, cout, st, pb, false, nullptr, nullptr, ksz));
    in = LANE(m->enc_a[j], e_out);
  }
  {
    ProfScope ps(m, 2);
    if (!exp_skip_small()) DV_TRY(launch_prelu_fwd(in, P + A.specs[A.enc_flat_al()].off, LANE(m->flat_a, A.flat), NB, A.flat, s));
  }
  return gconv_fprop(m, LANE(m->flat_a, A.flat), enc_dense_w(m), false, enc_dense_b(m),
                     nullptr, LANE(m->t, A.twp), nullptr, 1, NB, 1, A.flat, 1, A.twp, 1, 0, true);
}

static int decoder_forward(dv_model* m, int NB, bool keep_u) {
  if (m->bf.on) return bf_decoder_forward(m, NB, keep_u);
  const Arch& A = m->A;
  hipStream_t s = fwd_stream(m);
  float* P = m->P;
  {
    ProfScope ps(m, 2);
    // (dp > d: the slopes' 16-byte aligned slot is read past its d values; z's pad columns are zero, so are theirs)
    if (!exp_skip_small() && !m->ain_done)
      DV_TRY(launch_prelu_fwd(LANE(m->z, A.dp), P + A.specs[A.D0].off, LANE(m->dec_ain, A.dp), NB, A.dp, s));
    m->ain_done = false;
  }
  DV_TRY(gconv_fprop(m, LANE(m->dec_ain, A.dp), dec_dense0_w(m), false, P + A.specs[A.D0 + 2].off,
                     P + A.specs[A.D0 + 3].off, keep_u ? LANE(m->dec_uh, A.dec_hidden) : nullptr,
                     LANE(m->dec_ah, A.dec_hidden), 2, NB, 1, A.dp, 1, A.dec_hidden, 1, 0, true));
  int r = A.w0 * A.w0 * A.cfg.filters[A.L - 1];
  DV_TRY(gconv_fprop(m, LANE(m->dec_ah, A.dec_hidden), P + A.specs[A.D0 + 4].off, false, P + A.specs[A.D0 + 5].off,
                     P + A.specs[A.D0 + 6].off, keep_u ? LANE(m->dec_ur, r) : nullptr, LANE(m->dec_ar, r), 2, NB, 1,
                     A.dec_hidden, 1, r, 1, 0, true));
  const float* in = LANE(m->dec_ar, r);
  for (int j = 0; j < 2 * A.L; ++j) {
    int hin, cin, hout, cout, st;
    A.dec_layer(j, &hin, &cin, &hout, &cout, &st);
    const int ksz = A.dec_ksz(j);
    int pb = same_pad_before(hout, ksz, st, nullptr);
    const size_t e_out = (size_t)hout * hout * cout;
    // Conv2DTranspose = data gradient of a SAME conv over the output grid; kernel (kh,kw,cout,cin) is n-major
    DV_TRY(gconv_dgrad(m, in, P + A.specs[A.dec_k(j)].off, true, P + A.specs[A.dec_b(j)].off,
                       P + A.specs[A.dec_al(j)].off, keep_u ? LANE(m->dec_u[j], e_out) : nullptr,
                       LANE(m->dec_a[j], e_out), exp_epi(keep_u, hout), NB, hin, cin, hout, cout, st, pb, nullptr, nullptr, ksz));
    in = LANE(m->dec_a[j], e_out);
  }
  return gconv_fprop(m, in, m->Whp, false, m->bhp, nullptr, LANE(m->tpre, (size_t)A.dec_out * A.dec_out * A.C2p),
                     nullptr, 1, NB, A.dec_out, A.cfg.filters[0], A.dec_out, A.C2p, 1, 1);
}

// eps of the lane is already in m->eps when gen == false
static int sampler_forward(dv_model* m, int NB, bool gen, uint64_t seed, unsigned stream_id, unsigned row0,
                           bool want_std, int rep_nb = 0) {
  const Arch& A = m->A;
  SamplerParams sp;
  memset(&sp, 0, sizeof sp);
  sp.t = LANE(m->t, A.twp);
  sp.eps = LANE(m->eps, A.dp);
  sp.z = LANE(m->z, A.dp);
  sp.ldt = A.twp;
  sp.ldz = A.dp;
  sp.kl = LANE(m->kl, 1);
  sp.stddev = want_std ? LANE(m->zstd, A.dp) : nullptr;
  sp.NB = NB;
  sp.d = A.d;
  sp.diag_shift = A.cfg.diag_shift;
  sp.gen = gen ? 1 : 0;
  sp.seed = seed;
  sp.stream = stream_id;
  sp.row0 = row0 + (unsigned)m->b0;
  sp.rep_nb = rep_nb;
  sp.seed_ptr = m->use_seed_dev ? m->seed_dev : nullptr;
  if (m->bf.on && m->bf.t_nslab > 0) {           // the encoder Dense left K-split slabs: this launch is their finish
    sp.slab = m->bf.tslab;
    sp.nslab = m->bf.t_nslab;
    sp.slab_stride = (long)m->bf.NBp * m->bf.TWn;
    sp.lds = m->bf.TWn;
    sp.tbias = m->P + A.specs[A.enc_db()].off;
    sp.t_out = LANE(m->t, A.twp);
    m->bf.t_nslab = 0;
  }
  // the PReLU in front of the decoder's first Dense rides along (same formula, same bits as prelu_fwd_kernel)
  sp.alpha_in = m->P + A.specs[A.D0].off;
  sp.ain = LANE(m->dec_ain, A.dp);
  m->ain_done = true;
  ProfScope ps(m, 2);
  return A.d > 64 ? launch_sampler_wide_fwd(sp, fwd_stream(m)) : launch_sampler_fwd(sp, fwd_stream(m));
}

// head of the lane: per-block loss partials at part_off (blocks), optionally d(loss)/d(tpre) into gA
static void head_params(dv_model* m, HeadParams& hp, const float* ysrc, const int* idx, int first, int NB, int Bg,
                        bool want_grad, bool want_out, int part_block0) {
  const Arch& A = m->A;
  const size_t head_e = (size_t)A.dec_out * A.dec_out * A.C2p, stamp = (size_t)A.H * A.H * A.C;
  memset(&hp, 0, sizeof hp);
  hp.tpre = LANE(m->tpre, head_e);
  hp.y = ysrc;
  hp.idx = idx ? idx + m->b0 : nullptr;
  hp.first = first + m->b0;
  hp.dt = want_grad ? LANE(m->gA, head_e) : nullptr;
  hp.loc = want_out ? LANE(m->loc, stamp) : nullptr;
  hp.scale = want_out ? LANE(m->scale, stamp) : nullptr;
  hp.part = m->ws3 + (size_t)part_block0 * 2;
  hp.NB = NB;
  hp.Hd = A.dec_out;
  hp.H = A.H;
  hp.nb = A.C;
  hp.crop0 = A.crop0;
  hp.ld = A.C2p;
  hp.sigma_floor = A.cfg.sigma_floor;
  hp.gscale = (float)(1.0 / ((double)Bg * A.H * A.H * A.C));
  hp.mse_sample = m->mse_sample ? 1 : 0;
  hp.mse_row0 = m->b0;
  hp.mse_stream = DV_MSE_STREAM + (unsigned)m->ctx->rank;
  hp.mse_seed = m->cur_seed;
}

static int head_lane(dv_model* m, const float* ysrc, const int* idx, int first, int NB, int Bg, bool want_grad,
                     bool want_out, int part_block0, int* nblk) {
  if (m->bf.on) return bf_head_lane(m, ysrc, idx, first, NB, Bg, want_grad, want_out, part_block0, nblk);
  HeadParams hp;
  head_params(m, hp, ysrc, idx, first, NB, Bg, want_grad, want_out, part_block0);
  ProfScope ps(m, 2);
  return launch_head(hp, fwd_stream(m), nblk);
}

// Whole forward pass of a step: BN statistics over the full batch, then the batch runs as one lane or (large batches)
// as two half-batch lanes on the main and the aux stream, whose kernels fill each other's tails and store phases;
// the loss sums are reduced after the join.  ysrc == null: inference outputs only.
static int forward_all(dv_model* m, const float* xsrc, const float* ysrc, const int* idx, int first, int NB, int Bg,
                       bool training, bool upd_moving, bool keep_u, const float* eps_host, uint64_t seed,
                       unsigned stream_id, unsigned row0, bool want_std, bool want_grad, bool want_out,
                       bool run_encoder = true) {
  const Arch& A = m->A;
  dv_ctx* cx = m->ctx;
  hipStream_t s = cx->stream;
  m->cur_seed = seed;
  if (!m->bf.on) DV_TRY(wino_refresh_all(m, s));   // before the lanes split: both read the same transformed weights
#ifdef DV_DEBUG_EXPORTS
  if (!m->exp_deferred.empty()) {                  // DV_EXP_DEFER_WGRAD: see backward()
    if (ysrc && want_grad && cx->aux_stream) {
      m->wstream = cx->aux_stream;
      m->main_marked = false;
      for (auto& f : m->exp_deferred) DV_TRY(f());
      if (m->bf.on) DV_TRY(bf_flush_wred(m, nullptr));
      m->wstream = s;
    }
    m->exp_deferred.clear();
  }
#endif
  if (run_encoder) DV_TRY(bn_prepare(m, xsrc, idx, first, NB, Bg, training, upd_moving));
  if (eps_host) DV_TRY(copy_rows(m->eps, A.dp, eps_host, A.d, A.d, NB, hipMemcpyHostToDevice, s));
  const long head_blocks_total = ((long)NB * A.dec_out * A.dec_out + 255) / 256 + 2;
  if ((size_t)head_blocks_total * 2 > m->ws3_elems) {
    set_error("head workspace too small");
    return E_STATE;
  }
  // One lane by default since round 3: the Winograd kernels are persistent, one workgroup per CU with the CU's whole LDS,
  // so two half-batch lanes on two streams no longer fill gaps of each other - they queue (measured 4.885 ms with two
  // lanes, 4.827 ms with one, same box).  DV_FWD_LANES=n forces n; batches above the per-launch limit still split below.
  static const int want_lanes = getenv("DV_FWD_LANES") ? atoi(getenv("DV_FWD_LANES")) : 1;
  int nlanes = (m->split_forward && !m->prof_on && !m->bf.on && cx->aux_stream && NB >= 64) ? std::max(1, std::min(want_lanes, 4)) : 1;
  while (nlanes > 1 && NB / nlanes < 32) --nlanes;
  while (nlanes > 2 && !cx->lane_stream[nlanes - 3]) --nlanes;
  // The fp32 kernels address a launch's tensors with 32-bit byte offsets (2^30 elements: 8191 stamps of the 59-pixel
  // net, 2047 of a 128-pixel one).  A forward pass over more stamps - deblend() at BASELINE configs[4]'s batch of 8192 -
  // runs as lanes of at most that many stamps, each launch addressing its own lane; the backward pass has no lanes, so
  // training steps stay within the limit (check_step_args).
  if (!m->bf.on && m->Bc > 0) {
    const size_t per_stamp = std::max<size_t>(1, m->max_act_elems / (size_t)m->Bc);
    const long cap = (long)((((size_t)1 << 30) - 1) / per_stamp) & ~31L;
    if (NB > cap) {
      if (keep_u || !cx->aux_stream) {
        set_error("batch %d exceeds the %ld stamps one fp32 launch can address; lower the batch", NB, cap);
        return E_INVALID;
      }
      nlanes = (int)((NB + cap - 1) / cap);
      if (nlanes > 4 || (nlanes > 2 && !cx->lane_stream[nlanes - 3])) {
        set_error("batch %d needs %d forward lanes of <= %ld stamps; at most %d are available (DV_FWD_LANES)", NB, nlanes,
                  cap, cx->lane_stream[1] ? 4 : (cx->lane_stream[0] ? 3 : 2));
        return E_INVALID;
      }
    }
  }
  const int per = nlanes > 1 ? ((NB / nlanes + 31) / 32) * 32 : NB;   // lane sizes: multiples of 32 stamps
  int blk_done = 0, st = OK;
  // lane 0 runs on the main stream, lane 1 on the aux stream, further lanes on their own streams
  hipStream_t lstream[4] = {nullptr, cx->aux_stream, cx->lane_stream[0], cx->lane_stream[1]};
  if (nlanes > 1) {
    DV_HIP(hipEventRecord(cx->ev_ready, s));
    for (int lane = 1; lane < nlanes; ++lane) DV_HIP(hipStreamWaitEvent(lstream[lane], cx->ev_ready, 0));
  }
  for (int lane = 0; lane < nlanes && st == OK; ++lane) {
    m->b0 = lane * per;
    m->lane_id = lane;
    m->cs = lstream[lane];
    const int nb = std::min(per, NB - m->b0);
    if (nb <= 0) break;
    int nblk = 0;
    if (run_encoder) st = encoder_forward(m, xsrc, idx, first, nb, keep_u, /*defer_t=*/true);
    if (st == OK && run_encoder) st = sampler_forward(m, nb, eps_host == nullptr, seed, stream_id, row0, want_std);
    if (st == OK && m->bf.on) bf_head_fuse_request(m, ysrc, idx, first, nb, Bg, want_grad, want_out, blk_done);
    if (st == OK) st = decoder_forward(m, nb, keep_u);
    if (st == OK) st = head_lane(m, ysrc, idx, first, nb, Bg, want_grad, want_out, blk_done, &nblk);
    blk_done += nblk;
    if (st == OK && lane > 0) {
      if (hipEventRecord(cx->ev_lane[lane - 1], lstream[lane]) != hipSuccess ||
          hipStreamWaitEvent(s, cx->ev_lane[lane - 1], 0) != hipSuccess)
        st = E_HIP;
    }
  }
  m->b0 = 0;
  m->lane_id = 0;
  m->cs = nullptr;
  if (st != OK) return st;
  const int blk0 = blk_done, blk1 = 0;
  if (ysrc && m->defer_loss_sums) {
    m->loss_blocks = blk0 + blk1;
    m->loss_NB = NB;
    m->loss_pending = true;
  } else if (ysrc && !(exp_skip_tail() & 2)) {
    ProfScope ps(m, 2, s);
    DV_TRY(launch_reduce_rows_f64(m->ws3, blk0 + blk1, 2, m->scal, 1.0f, s));
    DV_TRY(launch_reduce_rows_f64(m->kl, NB, 1, m->scal + 2, 1.0f, s));
  }
  return OK;
}
#undef LANE

// ---- backward ---------------------------------------------------------------------------------
static int adam_range(dv_model* m, size_t beg, size_t end, hipStream_t st);

// First flat offset of the encoder's deep half (conv L .. dense): the start of the middle gradient bucket, or
// n_enc_train when the layout does not allow one (then the whole encoder goes into the final bucket).
static size_t enc_bucket_split(const Arch& A) {
  if (A.L < 2) return A.n_enc_train;
  const int k0 = A.enc_k(A.L);
  const size_t split = A.specs[k0].off;
  if (split >= A.n_enc_train || (split & 3)) return A.n_enc_train;
  for (int k = 0; k < (int)A.specs.size(); ++k) {
    const auto& sp = A.specs[k];
    if (!sp.trainable || sp.off >= A.n_enc_train) continue;
    if (k < k0 ? sp.off + sp.count > split : sp.off < split) return A.n_enc_train;
  }
  return split;
}

static int backward(dv_model* m, int NB, int Bg, const float* xsrc, const int* idx, int first) {
  if (m->bf.on) return bf_backward(m, NB, Bg);
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  float* P = m->P;
  float* G = m->G;
  const bool dg = m->dec_trainable;  // decoder parameter gradients wanted
  // The activation gradient walks down the chain through three rotating buffers.  Weight-gradient kernels run
  // on the aux stream beside the data-gradient chain; a buffer is only overwritten after the weight-gradient
  // launch that read it has been waited for (ev_buf), which with three buffers is two layers later.
  dv_ctx* cx = m->ctx;
  const bool ovl = m->overlap_wgrad && !m->prof_on && cx->aux_stream != nullptr;
  m->wstream = ovl ? cx->aux_stream : s;
  m->arena_off = 0;
  if (ovl) ensure_step_pool(m);
  // "no reuse" mode: as many buffers as data-gradient launches, so nothing below ever waits (or records)
  const int K = (ovl && (int)m->gbufs.size() >= 4 * A.L + 10) ? (int)m->gbufs.size() : 3;
  const bool no_reuse = K > 3;
  m->ws_count = 0;
  m->wino_wcount = 0;
  m->ws_last_rs = nullptr;
  m->main_marked = false;
  float* const* bufs = m->gbufs.data();
  bool pend[3] = {false, false, false};
  int ci = 0;                        // bufs[0] holds d(tpre)
  float* cur = bufs[0];
  float* oth = nullptr;
  auto next_out = [&]() -> int {     // pick the output buffer of the next data-gradient launch
    const int o = (ci + 1) % K;
    m->main_marked = false;
    if (no_reuse) {
      if (o == 0) return -2;         // wrapped: more launches than buffers
      oth = bufs[o];
      return o;
    }
    if (pend[o]) {
      if (hipStreamWaitEvent(s, cx->ev_buf[o], 0) != hipSuccess) return -1;
      pend[o] = false;
    }
    oth = bufs[o];
    return o;
  };
  auto wgrad_read = [&]() -> int {   // the weight-gradient launch just queued reads bufs[ci]
    if (!ovl || no_reuse) return OK;
    if (hipEventRecord(cx->ev_buf[ci], cx->aux_stream) != hipSuccess) return E_HIP;
    pend[ci] = true;
    return OK;
  };
  auto advance = [&]() {             // the data gradient just written becomes the current one
    ci = (ci + 1) % K;
    cur = bufs[ci];
  };
#define DV_NEXT_OUT()                                  \
  do {                                                 \
    if (next_out() < 0) {                              \
      set_error("data-gradient buffer hand-over failed"); \
      return E_HIP;                                    \
    }                                                  \
  } while (0)
  const int Hd = A.dec_out, f0 = A.cfg.filters[0], C2 = 2 * A.C, C2p = A.C2p;
  // head conv (stored with C2p output channels; the pad channels carry zeros)
#ifdef DV_DEBUG_EXPORTS
  // DV_EXP_DEFER_WGRAD=n (MEASUREMENT only: the optimizer runs before these gradients exist): the kernel gradients of the
  // head conv and of the last n transposed convs are held back and queued on the weight-gradient stream at the start of the
  // NEXT forward pass, whose encoder has no second stream beside it - what a cross-step pipeline of the decoder's late
  // layers could gain
  static const int exp_defer = DV_EXP_SWITCH("DV_EXP_DEFER_WGRAD");
#else
  [[maybe_unused]] constexpr int exp_defer = 0;
#endif
  if (dg) {
    hipStream_t ws = m->wstream ? m->wstream : s;
    auto head_wg = [=]() -> int {
      DV_TRY(wgrad(m, m->dec_a[2 * A.L - 1], Hd, f0, cur, Hd, C2p, NB, 1, 1, false, m->Ghs, f0, f0));
      DV_TRY(wgrad_result_ready(m, ws));
      ProfScope ps(m, 2, ws);
      DV_TRY(launch_take_cols(m->Ghs, G + A.specs[A.head_k()].off, 9 * f0, C2p, C2, ws));
      return OK;
    };
#ifdef DV_DEBUG_EXPORTS
    if (exp_defer > 0 && no_reuse && ovl) m->exp_deferred.push_back(head_wg);
    else
#endif
      DV_TRY(head_wg());
    DV_TRY(wgrad_read());
    if (!(exp_skip_tail() & 2)) DV_TRY(bias_grad_colsum(m, cur, (long)NB * Hd * Hd, C2p, C2, A.head_b()));
  }
  bool cur_is_du = false;   // true when the data-gradient launch already applied the PReLU backward of `cur`'s layer
  {
    const int jl = 2 * A.L - 1;
    FuseBwd fz{m->dec_u[jl], A.dec_al(jl), A.dec_b(jl), dg};
    DV_NEXT_OUT();
    DV_TRY(gconv_dgrad(m, cur, m->Whp, true, nullptr, nullptr, oth, nullptr, 0, NB, Hd, C2p, Hd, f0, 1, 1, &fz,
                       &cur_is_du));
    advance();
  }
  // decoder conv-transpose stack
  for (int j = 2 * A.L - 1; j >= 0; --j) {
    int hin, cin, hout, cout, st;
    A.dec_layer(j, &hin, &cin, &hout, &cout, &st);
    const int ksz = A.dec_ksz(j);
    int pb = same_pad_before(hout, ksz, st, nullptr);
    if (!cur_is_du) DV_TRY(prelu_bwd(m, cur, m->dec_u[j], A.dec_al(j), A.dec_b(j), NB, hout * hout * cout, cout, dg));
    m->du_dec[j] = cur;
    const float* xin = j == 0 ? m->dec_ar : m->dec_a[j - 1];
    if (dg) {
      float* const gk = G + A.specs[A.dec_k(j)].off;
      const float* const dy = cur;
      auto layer_wg = [=]() -> int {
        return wgrad(m, dy, hout, cout, xin, hin, cin, NB, st, pb, false, gk, cout, cout, nullptr, false, ksz);
      };
#ifdef DV_DEBUG_EXPORTS
      if (exp_defer > 0 && j >= 2 * A.L - exp_defer && no_reuse && ovl) m->exp_deferred.push_back(layer_wg);
      else
#endif
        DV_TRY(layer_wg());
      DV_TRY(wgrad_read());
    }
    // d(input) = strided conv of d(pre-activation) with K[kh,kw,co,ci] (rows (tap,co), cols ci: k-major)
    DV_NEXT_OUT();
    if (j > 0) {   // the input of conv-transpose j is the PReLU output of conv-transpose j-1: fuse its backward
      FuseBwd fz{m->dec_u[j - 1], A.dec_al(j - 1), A.dec_b(j - 1), dg};
      DV_TRY(gconv_fprop(m, cur, P + A.specs[A.dec_k(j)].off, false, nullptr, nullptr, oth, nullptr, 0, NB, hout, cout,
                         hin, cin, st, pb, false, &fz, &cur_is_du, ksz));
    } else {
      DV_TRY(gconv_fprop(m, cur, P + A.specs[A.dec_k(j)].off, false, nullptr, nullptr, oth, nullptr, 0, NB, hout, cout,
                         hin, cin, st, pb, false, nullptr, nullptr, ksz));
      cur_is_du = false;
    }
    advance();
  }
  // dense trunk of the decoder
  int r = A.w0 * A.w0 * A.cfg.filters[A.L - 1];
  DV_TRY(prelu_bwd(m, cur, m->dec_ur, A.D0 + 6, A.D0 + 5, NB, r, r, dg));
  if (dg) {
    DV_TRY(wgrad(m, m->dec_ah, 1, A.dec_hidden, cur, 1, r, NB, 1, 0, true, G + A.specs[A.D0 + 4].off, 1, 1));
    DV_TRY(wgrad_read());
  }
  DV_NEXT_OUT();
  DV_TRY(gconv_fprop(m, cur, P + A.specs[A.D0 + 4].off, true, nullptr, nullptr, oth, nullptr, 0, NB, 1, r, 1,
                     A.dec_hidden, 1, 0, true));
  advance();
  DV_TRY(prelu_bwd(m, cur, m->dec_uh, A.D0 + 3, A.D0 + 2, NB, A.dec_hidden, A.dec_hidden, dg));
  if (dg) {
    DV_TRY(wgrad(m, m->dec_ain, 1, A.dp, cur, 1, A.dec_hidden, NB, 1, 0, true, dec_dense0_g(m), 1, 1));
    if (m->G0p) DV_TRY(take_padded_grad(m, m->G0p, G + A.specs[A.D0 + 1].off, 1, A.dp * A.dec_hidden, A.d * A.dec_hidden));
    DV_TRY(wgrad_read());
  }
  DV_NEXT_OUT();
  DV_TRY(gconv_fprop(m, cur, dec_dense0_w(m), true, nullptr, nullptr, oth, nullptr, 0, NB, 1, A.dec_hidden,
                     1, A.dp, 1, 0, true));
  advance();
  DV_TRY(prelu_bwd(m, cur, m->z, A.D0, -1, NB, A.dp, A.dp, dg));
  // every decoder gradient is final here and no later kernel of the step reads a decoder parameter: the bucket is
  // all-reduced on the comm stream while the encoder backward runs, and (early_adam) updated there right behind it
  const bool early = m->early_adam && ovl;
  if ((m->ctx->comm || early) && dg && A.n_train > A.n_enc_train) {
    DV_HIP(hipEventRecord(m->ctx->ev_dec, s));
    DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, m->ctx->ev_dec, 0));
    if (ovl) {                                       // ... and the decoder weight gradients on the aux stream
      DV_HIP(hipEventRecord(cx->ev_join, cx->aux_stream));
      DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, cx->ev_join, 0));
      DV_HIP(hipEventRecord(cx->ev_red, cx->red_stream));   // ... and the d(alpha) / d(bias) reductions
      DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, cx->ev_red, 0));
    }
    if (m->ctx->comm)
      DV_TRY(comm_allreduce(m->ctx, G + A.n_enc_train, A.n_train - A.n_enc_train));
    if (early && m->opt_dec) {
      DV_TRY(adam_range(m, A.n_enc_train, A.n_train, cx->comm_stream));
      DV_TRY(refresh_head_pad(m, cx->comm_stream));
      m->adam_done_from = A.n_enc_train;
    }
  }
  m->enc_reduced_from = A.n_enc_train;
  // sampler + KL
  float kls = (float)((double)A.cfg.kl_multiplicity * A.cfg.kl_weight / ((double)Bg * (double)Bg));
  {
    ProfScope ps(m, 2);
    DV_NEXT_OUT();
    DV_TRY((A.d > 64 ? launch_sampler_wide_bwd : launch_sampler_bwd)(m->t, m->eps, m->z, cur, oth, NB, A.d, A.twp, A.dp,
                                                                   A.cfg.diag_shift, kls, s));
  }
  advance();  // cur = d(t) [NB, twp]
  // encoder dense
  DV_TRY(bias_grad_colsum(m, cur, NB, A.twp, A.tw, A.enc_db()));
  DV_TRY(wgrad(m, m->flat_a, 1, A.flat, cur, 1, A.twp, NB, 1, 0, true, enc_dense_g(m), 1, 1));
  if (m->Gdp) DV_TRY(take_padded_grad(m, m->Gdp, G + A.specs[A.enc_dk()].off, A.flat, A.twp, A.tw));
  DV_TRY(wgrad_read());
  DV_NEXT_OUT();
  DV_TRY(gconv_fprop(m, cur, enc_dense_w(m), true, nullptr, nullptr, oth, nullptr, 0, NB, 1, A.twp, 1,
                     A.flat, 1, 0, true));
  advance();
  DV_TRY(prelu_bwd(m, cur, m->enc_a[2 * A.L - 1], A.enc_flat_al(), -1, NB, A.flat, A.flat, true));
  cur_is_du = false;
  for (int j = 2 * A.L - 1; j >= 0; --j) {
    int hin, cin, hout, cout, st;
    A.enc_layer(j, &hin, &cin, &hout, &cout, &st);
    const int ksz = A.enc_ksz(j);
    int pb = same_pad_before(hin, ksz, st, nullptr);
    // first layer: its PReLU backward is folded into the weight-gradient kernel (no data gradient follows it)
    const bool fuse0 = j == 0 && !cur_is_du && m->fuse_first && cout == 32 && st == 1 && pb == 1 && ksz == 3 && !g_no_special &&
                       A.C0p == 8 && wgrad_strip8_fusable(hout, hout);     // (the fused strip form reads 8-channel input rows)
    if (!cur_is_du && !fuse0)
      DV_TRY(prelu_bwd(m, cur, m->enc_u[j], A.enc_al(j), A.enc_b(j), NB, hout * hout * cout, cout, true));
    m->du_enc[j] = fuse0 ? nullptr : cur;      // (fused first layer: d(pre-activation) is never materialised,
    if (j == 0) m->da_enc0 = fuse0 ? cur : nullptr;   //  its d(activation) is what the pass leaves)
    const float* xin = j == 0 ? m->xn : m->enc_a[j - 1];
    int cin_phys = j == 0 ? A.C0p : cin;
    if (j == 0) {
      // first conv + input BatchNorm: the gradient w.r.t. the folded 8-channel kernel gives d(kernel), d(gamma) and
      // d(beta) directly (bn_conv0_grads_kernel), so this layer needs no data-gradient pass at all
      // the last weight gradient of the step goes to the main stream, which would otherwise idle while the aux
      // stream works off its backlog
      const bool last_on_main = true;
      hipStream_t ws = (m->wstream && !last_on_main) ? m->wstream : s;
      FuseBwd f0{m->enc_u[0], A.enc_al(0), A.enc_b(0), true};
      DV_TRY(wgrad(m, xin, hin, A.C0p, cur, hout, cout, NB, st, pb, false, m->G0s, A.C0p, A.C0p, fuse0 ? &f0 : nullptr,
                   last_on_main, ksz));
      if (exp_skip_tail() & 1) break;
      DV_TRY(wgrad_result_ready(m, ws));
      ProfScope ps(m, 2, ws);
      DV_TRY(launch_bn_conv0_grads(m->G0s, P + A.specs[A.enc_k(0)].off, P + A.specs[0].off, P + A.specs[1].off,
                                   G + A.specs[A.enc_k(0)].off, G + A.specs[0].off, G + A.specs[1].off, ksz * ksz, A.C,
                                   A.C0p, cout, ws));
      DV_TRY(wgrad_read());
      break;
    }
    DV_TRY(wgrad(m, xin, hin, cin_phys, cur, hout, cout, NB, st, pb, false, G + A.specs[A.enc_k(j)].off, cin_phys,
                 cin_phys, nullptr, false, ksz));
    DV_TRY(wgrad_read());
    const float* W = P + A.specs[A.enc_k(j)].off;
    DV_NEXT_OUT();
    FuseBwd fz{m->enc_u[j - 1], A.enc_al(j - 1), A.enc_b(j - 1), true};   // j >= 1 here (j == 0 left the loop above)
    DV_TRY(gconv_dgrad(m, cur, W, true, nullptr, nullptr, oth, nullptr, 0, NB, hout, cout, hin, cin_phys, st, pb, &fz,
                       &cur_is_du, ksz));
    advance();
    if ((cx->comm || early) && j == A.L && A.L >= 2) {
      // Middle bucket: the gradients of the deep half of the encoder (conv L .. conv 2L-1, their PReLUs, the
      // flatten PReLU and the dense layer - 13.8 of the encoder's 15 MB) are final once this layer's weight-gradient
      // work has been queued, and its data-gradient kernel (just queued) was the last reader of those parameters.
      // They are all-reduced - and with early_adam updated - while the shallow half is still being differentiated,
      // so that only a ~1 MB bucket is left for the end of the step.
      const size_t split = enc_bucket_split(A);
      if (split < A.n_enc_train) {
        hipStream_t ws = m->wstream ? m->wstream : s;
        DV_HIP(hipEventRecord(cx->ev_mid, ws));      // kernel gradients are written on this stream,
        DV_HIP(hipStreamWaitEvent(cx->comm_stream, cx->ev_mid, 0));
        if (ovl) {                                   // d(alpha) / d(bias) on the reduction stream,
          DV_HIP(hipEventRecord(cx->ev_red, cx->red_stream));
          DV_HIP(hipStreamWaitEvent(cx->comm_stream, cx->ev_red, 0));
          DV_HIP(hipEventRecord(cx->ev_dec, s));     // and the main stream has finished reading the parameters
          DV_HIP(hipStreamWaitEvent(cx->comm_stream, cx->ev_dec, 0));
        }
        if (cx->comm) {
          DV_TRY(comm_allreduce(cx, G + split, A.n_enc_train - split));
          m->enc_reduced_from = split;
        }
        if (early && m->opt_enc) {
          DV_TRY(adam_range(m, split, A.n_enc_train, cx->comm_stream));
          m->adam_done_from = std::min(m->adam_done_from, split);
        }
      }
    }
  }
  if (ovl) {                                         // join: every parameter gradient is final past this point
    DV_HIP(hipEventRecord(cx->ev_join, cx->aux_stream));
    DV_HIP(hipStreamWaitEvent(s, cx->ev_join, 0));
    DV_HIP(hipEventRecord(cx->ev_red, cx->red_stream));
    DV_HIP(hipStreamWaitEvent(s, cx->ev_red, 0));
  }
  m->wstream = s;
  m->du_valid = no_reuse;        // (with three rotating buffers the tensors have been overwritten by now)
#undef DV_NEXT_OUT
  return OK;
}

#include "engine_bf16.inl"

// legacy Adam on the flat range [beg, end) (clipped to what this model is training), on stream st
static int adam_range(dv_model* m, size_t beg, size_t end, hipStream_t st) {
  const Arch& A = m->A;
  beg = std::max(beg, m->opt_enc ? (size_t)0 : A.n_enc_train);
  end = std::min(end, m->opt_dec ? A.n_train : A.n_enc_train);
  if (end <= beg) return OK;
  ProfScope ps(m, 2, st);
  return launch_adam(m->P + beg, m->Mm + beg, m->Vv + beg, m->G + beg, (long)(end - beg), m->lr_t_step, m->b1, m->b2,
                     m->aeps, st);
}

static void begin_update(dv_model* m) {     // step counter and bias-corrected step size of this update
  m->iter += 1;
  const double t = (double)m->iter;
  m->lr_t_step = (float)((double)m->lr * sqrt(1.0 - pow((double)m->b2, t)) / (1.0 - pow((double)m->b1, t)));
}

// what is left of the update at the end of the step: the ranges below adam_done_from, then the derived tensors
static int optimizer_step(dv_model* m) {
  const Arch& A = m->A;
  if (exp_skip_tail() & 1) {
    m->bf.dirty_mask = 0;
    m->bf.early_cast = 0;
    return OK;
  }
  DV_TRY(adam_range(m, 0, std::min(m->adam_done_from, A.n_train), m->ctx->stream));
  m->param_epoch++;
  if (m->opt_enc) DV_TRY(refresh_w1p(m));
  if (m->opt_dec && m->adam_done_from > A.n_enc_train) DV_TRY(refresh_head_pad(m));
  m->bf.dirty_mask = 7 & ~m->bf.early_cast;     // (the buckets updated on the comm stream were re-cast there)
  m->bf.early_cast = 0;
  return OK;
}

enum StepMode { MODE_TRAIN = 0, MODE_EVAL = 1, MODE_GRAD = 2 };

static int check_step_args(dv_model* m, int slot, const int32_t* idx, int64_t first, int B) {
  if (!m) {
    set_error("null model");
    return E_INVALID;
  }
  if (slot < 0 || slot > 1 || (!m->slots[slot].x && !m->slots[slot].streamed)) {
    set_error("data slot %d is empty (call dv_data_upload or dv_data_stream_open first)", slot);
    return E_STATE;
  }
  if (B < 1 || B > m->Bc) {
    set_error("batch %d outside [1, max_batch=%d]", B, m->Bc);
    return E_INVALID;
  }
  if (!idx && (first < 0 || first + B > m->slots[slot].n)) {
    set_error("rows [%lld, %lld) outside the %lld uploaded stamps", (long long)first, (long long)(first + B),
              (long long)m->slots[slot].n);
    return E_INVALID;
  }
  if (idx)
    for (int i = 0; i < B; ++i)
      if (idx[i] < 0 || idx[i] >= m->slots[slot].n) {
        set_error("index %d out of range", idx[i]);
        return E_INVALID;
      }
  return OK;
}

// Batch sums of the input BatchNorm for the step that will read rows [first, first + NB) of `x`: queued on the comm
// stream (idle between the collectives), all-reduced there, consumed by bn_prepare() of that step.
// Batch sums of the input BatchNorm for a batch that is about to be (idx_host != null: the step being queued, whose
// index vector is copied to idx_dev on the comm stream first) or will next be (contiguous rows from `first`) trained
// on, computed on the comm stream while the previous step still runs.
static int bn_prefetch(dv_model* m, const float* x, int64_t first, int NB, int Bg, int* idx_dev = nullptr,
                       const int32_t* idx_host = nullptr) {
  const Arch& A = m->A;
  dv_ctx* c = m->ctx;
  if (!m->bn_pre_part || !c->comm_stream) return OK;
  const int HW = A.H * A.H;
  int nblk = 0;
  // the previous consumer of bn_pre_sums (the bn_finalize of the step that used them) recorded ev_bnpre_go behind it
  DV_HIP(hipStreamWaitEvent(c->comm_stream, m->ev_bnpre_go, 0));
  if (idx_host)
    DV_HIP(hipMemcpyAsync(idx_dev, idx_host, (size_t)NB * sizeof(int), hipMemcpyHostToDevice, c->comm_stream));
  if (((size_t)NB * HW + 1023) / 1024 * (2 * DV_BN_MAXC) > m->bn_pre_part_elems) {      // before the launch, not after it has written
    set_error("bn prefetch workspace too small");
    return E_STATE;
  }
  DV_TRY(launch_bn_stats(x, idx_dev, (int)first, NB, HW, A.C, m->bn_pre_part, &nblk, c->comm_stream));
  DV_TRY(launch_reduce_rows_f64(m->bn_pre_part, nblk, 2 * DV_BN_MAXC, m->bn_pre_sums, 1.0f, c->comm_stream));
  if (c->comm) DV_TRY(comm_allreduce(c, m->bn_pre_sums, 2 * DV_BN_MAXC));
  static const bool no_input_ahead = getenv("DV_NO_INPUT_AHEAD") != nullptr;
  if (m->bf.on && m->bf.xh_alt && !no_input_ahead) {
    // bf16 engine: the whole head of the step - statistics -> bn_finalize (this is a TRAINING step: batch statistics, moving
    // statistics updated) -> normalised stamp-inner input - runs here, into the buffer the step in flight does not read
    float* P = m->P;
    DV_TRY(launch_bn_finalize(m->bn_pre_sums, (float)((double)Bg * HW), A.C, P + A.specs[0].off, P + A.specs[1].off,
                              P + A.specs[2].off, P + A.specs[3].off, A.cfg.bn_eps, A.cfg.bn_momentum,
                              A.cfg.bn_moving_var_unbiased, 1, 1, m->bnstate, c->comm_stream));
    DV_TRY(launch_bf_input(x, idx_dev, (int)first, NB, (NB + 15) & ~15, HW, A.C, m->bnstate, m->bf.xh_alt, c->comm_stream));
    m->bf.in_pre = true;
  }
  DV_HIP(hipEventRecord(m->ev_bnpre, c->comm_stream));
  m->bn_pre_valid = true;
  m->bn_pre_x = x;
  m->bn_pre_idx = idx_dev;
  m->bn_pre_first = first;
  m->bn_pre_B = NB;
  return OK;
}

// enqueue one step (no host sync); scalars land in m->scal[0..2]
// `ds`: a resident slot, or the ring entry of a streamed batch (stream_stage), whose copy every reader waits for
static int enqueue_step(dv_model* m, StepMode mode, const DataSlot& ds, const int32_t* idx_host, int64_t first, int B,
                        int Bg, const float* eps_host, uint64_t seed) {
  hipStream_t s = m->ctx->stream;
  const int* idx = nullptr;
  if (idx_host) {
      if (mode == MODE_TRAIN && !m->prof_on && m->idx_slots && m->bn_pre_part && m->ctx->comm_stream &&
        m->overlap_wgrad) {
      // shuffled batches (fit): index vector and BN batch sums of THIS step go through the comm stream, which the
      // host reaches while the previous step is still running (steps are queued two ahead) - the forward pass below
      // then starts with bn_finalize instead of a statistics pass over the batch
      int* slotp = m->idx_slots + (size_t)(m->idx_slot_next++ & 3) * m->Bc;
      if (ds.ready) DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, ds.ready, 0));
      DV_TRY(bn_prefetch(m, ds.x, first, B, Bg, slotp, idx_host));
      idx = slotp;
    } else {
      DV_HIP(hipMemcpyAsync(m->idx_dev, idx_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
      idx = m->idx_dev;
    }
  }
  const bool training = mode != MODE_EVAL;
  const bool bwd = mode != MODE_EVAL;
  m->lastB = B;
  if (ds.ready) DV_HIP(hipStreamWaitEvent(s, ds.ready, 0));      // a streamed batch: its copy has landed
  // Philox stream: one counter row per (rank-local) stamp; ranks are separated through the stream id
  // loc / scale of a gradient or train step are only written on request (dv_model_set_keep_outputs: the parity
  // tests read them back) - 42 MB of stores per 256-stamp step that training has no reader for
  static const bool sums_on_main = getenv("DV_BF_SUMS_ON_MAIN") != nullptr;     // (A/B: the form until round 6)
  m->loss_pending = false;       // (a step that failed between its two passes leaves nothing behind for this one)
  m->defer_loss_sums = bwd && m->bf.on && bf_wstream(m) != s && m->arena_reduce && m->ctx->red_stream != nullptr && m->ws_head &&
                       !sums_on_main;
  const int fst = forward_all(m, ds.x, ds.y, idx, (int)first, B, Bg, training, mode == MODE_TRAIN, bwd, eps_host, seed,
                              (unsigned)m->ctx->rank, 0u, false, bwd, !bwd || m->keep_outputs);
  const bool sums_deferred = m->defer_loss_sums;
  m->defer_loss_sums = false;
  DV_TRY(fst);
  // the loss sums are only read after the step: with a backward pass the main stream joins the comm stream behind
  // the last gradient bucket anyway, so it does not stop here for this latency-bound collective
  // (sums_deferred: sums and collective are queued by bf_backward, on the reduction and the comm stream)
  if (!sums_deferred) DV_TRY(allreduce_small(m->ctx, m->scal, 4, !bwd));
  if (mode == MODE_TRAIN && m->hint_next_first >= 0 && !m->prof_on) {
    // fp32 engine: the statistics pass of the NEXT batch (35 us, HBM-bound, comm stream) is held until this forward pass
    // has drained: beside the forward's persistent one-workgroup-per-CU Winograd kernels it takes CU slots one of their
    // launches then finishes without (4.685 -> 4.655 ms per step, three alternating same-box runs; later gates - the
    // decoder trunk, the encoder trunk - 4.66 / 4.67).  The bf16 engine's forward kernels share a CU: no gate (2.09 ms
    // without, 2.11 with).
    if (!m->bf.on && m->ctx->comm_stream && !m->ctx->comm) {   // (with a communicator allreduce_small above is that gate)
      DV_HIP(hipEventRecord(m->ctx->ev_small, s));
      DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, m->ctx->ev_small, 0));
    }
    DV_TRY(bn_prefetch(m, ds.x, m->hint_next_first, B, Bg));
    m->hint_next_first = -1;
  }
  if (mode == MODE_TRAIN) begin_update(m);
  m->adam_done_from = m->A.n_train;
  static const bool no_early = getenv("DV_NO_EARLY_ADAM") != nullptr;
  m->early_adam = mode == MODE_TRAIN && !no_early && !m->prof_on;
  if (bwd) {
    DV_TRY(backward(m, B, Bg, ds.x, idx, (int)first));
    if (!m->ctx->comm && m->adam_done_from < m->A.n_train) {
      // parameter ranges were updated on the comm stream: everything after this step reads them
      DV_HIP(hipEventRecord(m->ctx->ev_comm, m->ctx->comm_stream));
      DV_HIP(hipStreamWaitEvent(s, m->ctx->ev_comm, 0));
    }
    if (m->ctx->comm) {
      // encoder bucket (the decoder bucket was queued inside backward()); the optimizer waits for both
      DV_HIP(hipEventRecord(m->ctx->ev_enc, s));
      DV_HIP(hipStreamWaitEvent(m->ctx->comm_stream, m->ctx->ev_enc, 0));
      if (m->enc_reduced_from > 0) DV_TRY(comm_allreduce(m->ctx, m->G, m->enc_reduced_from));
      DV_HIP(hipEventRecord(m->ctx->ev_comm, m->ctx->comm_stream));
      DV_TRY(main_waits_for_comm(m->ctx, m->ctx->ev_comm));
    }
  }
  if (mode == MODE_TRAIN) DV_TRY(optimizer_step(m));
  return OK;
}

static void scalars_from_sums(const dv_model* m, const float* h, int Bg, float* out);

static int fetch_scalars(dv_model* m, int Bg, float* out) {
  float h[4];
  DV_HIP(hipMemcpyAsync(h, m->scal, sizeof h, hipMemcpyDeviceToHost, m->ctx->stream));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  scalars_from_sums(m, h, Bg, out);
  return OK;
}

static void scalars_from_sums(const dv_model* m, const float* h, int Bg, float* out) {
  const Arch& A = m->A;
  double npix = (double)A.H * A.H * A.C;
  double nll_mean = (double)h[0] / ((double)Bg * npix);
  double mse = (double)h[1] / ((double)Bg * npix);
  double kl_reg = (double)A.cfg.kl_multiplicity * A.cfg.kl_weight * (double)h[2] / ((double)Bg * (double)Bg);
  if (out) {
    out[DV_S_LOSS] = (float)(nll_mean + kl_reg);
    out[DV_S_NLL_MEAN] = (float)nll_mean;
    out[DV_S_KL_REG] = (float)kl_reg;
    out[DV_S_MSE] = (float)mse;
  }
}

// Host threads that copy stamps between the caller's arrays and pinned memory (the inference pipe, the streamed slots):
// DV_COPY_THREADS, otherwise half the hardware threads, at most 8.
static int copy_threads() {
  const char* e = getenv("DV_COPY_THREADS");
  const int hw = (int)std::thread::hardware_concurrency();
  return e ? std::max(1, atoi(e)) : std::max(1, std::min(8, hw > 0 ? hw / 2 : 4));
}

// ---- streamed slots (StreamRing) ----------------------------------------------------------------------------------
static int ring_sync_streams(dv_model* m) {
  dv_ctx* c = m->ctx;
  for (hipStream_t st : {c->stream, c->aux_stream, c->red_stream, c->comm_stream, m->ring ? m->ring->copy : nullptr})
    if (st) DV_HIP(hipStreamSynchronize(st));
  return OK;
}

static void ring_free(dv_model* m) {
  delete m->ring;
  m->ring = nullptr;
}

// the ring of the model's max_batch; on failure nothing is left allocated
static int ring_get(dv_model* m) {
  if (m->ring) return OK;
  const Arch& A = m->A;
  std::unique_ptr<StreamRing> R(new StreamRing());
  const size_t E = (size_t)A.H * A.H * A.C;
  R->yoff = ((size_t)m->Bc * E + 63) & ~(size_t)63;
  const size_t floats = R->yoff + (size_t)m->Bc * E;
  // its own stream: on the comm stream a copy would queue behind the previous step's bucket all-reduces and early Adam
  DV_HIP(hipStreamCreateWithFlags(&R->copy, hipStreamNonBlocking));
  for (int r = 0; r < StreamRing::kDepth; ++r) {
    DV_TRY(R->dev[r].alloc(floats));
    DV_TRY(R->host[r].alloc(floats));
    DV_HIP(hipEventCreateWithFlags(&R->h2d[r], hipEventDisableTiming));    // copy -> kernels: system-scope release
    for (auto& e : R->rel[r]) DV_HIP(hipEventCreateWithFlags(&e, sync_event_flags()));   // ordering only
  }
  R->iota.resize(m->Bc);
  for (int i = 0; i < m->Bc; ++i) R->iota[i] = i;
  R->threads = copy_threads();
  m->ring = R.release();
  return OK;
}

// rows idx[0..B) (or first..first+B) of a streamed slot -> dx / dy as B contiguous float32 rows of E elements each; the
// float64 -> float32 cast is a C cast (round to nearest even, as numpy's astype).  x and y rows are split over the threads.
static void gather_rows(float* dx, float* dy, const DataSlot& ds, const int32_t* idx, int64_t first, int B, size_t E,
                        int threads) {
  auto work = [&](int lo, int hi) {
    for (int u = lo; u < hi; ++u) {
      const bool isy = u >= B;
      const int i = isy ? u - B : u;
      const int64_t row = idx ? (int64_t)idx[i] : first + i;
      const char* src = (isy ? ds.hy : ds.hx) + row * (isy ? ds.sy : ds.sx);
      float* dst = (isy ? dy : dx) + (size_t)i * E;
      if (isy ? ds.y64 : ds.x64) {
        const double* sd = reinterpret_cast<const double*>(src);
        for (size_t j = 0; j < E; ++j) dst[j] = (float)sd[j];
      } else {
        memcpy(dst, src, E * sizeof(float));
      }
    }
  };
  const int units = 2 * B;
  threads = std::max(1, std::min(threads, units));
  if (threads == 1 || (size_t)units * E < (size_t)1 << 18) {
    work(0, units);
    return;
  }
  std::vector<std::thread> pool;
  const int per = (units + threads - 1) / threads;
  for (int t = 1; t < threads; ++t) {
    const int lo = std::min(units, per * t), hi = std::min(units, per * (t + 1));
    if (lo < hi) pool.emplace_back(work, lo, hi);
  }
  work(0, std::min(units, per));
  for (auto& th : pool) th.join();
}

// Gathers the batch of one step of streamed slot `ds` into the next ring entry's pinned staging and queues its copy to
// HBM on the copy stream (hazards: StreamRing).  *view addresses the batch as rows 0..B of a resident slot whose readers
// wait for the copy; *entry is the ring entry, to be released with stream_release once the step is queued.
static int stream_stage(dv_model* m, DataSlot& ds, const int32_t* idx, int64_t first, int B, DataSlot* view, int* entry) {
  StreamRing* R = m->ring;
  const Arch& A = m->A;
  const size_t E = (size_t)A.H * A.H * A.C;
  const int r = (int)(R->next % StreamRing::kDepth);
  if (R->queued[r]) DV_HIP(hipEventSynchronize(R->h2d[r]));     // the pinned entry's previous copy has been read
  gather_rows(R->host[r], R->host[r] + R->yoff, ds, idx, first, B, E, R->threads);
  if (R->queued[r])
    for (auto e : R->rel[r]) DV_HIP(hipStreamWaitEvent(R->copy, e, 0));   // every reader of the entry's last batch is done
  const size_t bytes = (size_t)B * E * sizeof(float);
  DV_HIP(hipMemcpyAsync(R->dev[r], R->host[r], bytes, hipMemcpyHostToDevice, R->copy));
  DV_HIP(hipMemcpyAsync(R->dev[r] + R->yoff, R->host[r] + R->yoff, bytes, hipMemcpyHostToDevice, R->copy));
  DV_HIP(hipEventRecord(R->h2d[r], R->copy));
  R->next += 1;
  ds.h2d_bytes += 2 * (int64_t)bytes;
  *view = DataSlot();
  view->x = R->dev[r];
  view->y = R->dev[r] + R->yoff;
  view->n = B;
  view->ready = R->h2d[r];
  *entry = r;
  return OK;
}

// records the release events of ring entry r behind everything queued so far on the streams that read a step's batch
static int stream_release(dv_model* m, int r) {
  StreamRing* R = m->ring;
  dv_ctx* c = m->ctx;
  const hipStream_t readers[StreamRing::kRel] = {c->stream, c->aux_stream ? c->aux_stream : c->stream,
                                                 c->comm_stream ? c->comm_stream : c->stream,
                                                 c->red_stream ? c->red_stream : c->stream};
  for (int k = 0; k < StreamRing::kRel; ++k) DV_HIP(hipEventRecord(R->rel[r][k], readers[k]));
  R->queued[r] = true;
  return OK;
}

// Queues one step on `slot`.  A streamed slot's rows are gathered and copied first; the step then reads them as rows
// 0..B of the ring entry - through the identity index vector when the caller named rows by index, so that the step takes
// exactly the kernels (and the comm-stream prefetch) the same batch takes on a resident slot.  idx_pinned (the deferred
// step): the index vector the step reads is staged there, because the caller's may be gone before its copy runs.
static int enqueue_slot_step(dv_model* m, StepMode mode, int slot, const int32_t* idx, int64_t first, int B, int Bg,
                             const float* eps, uint64_t seed, int* idx_pinned = nullptr) {
  DataSlot& ds = m->slots[slot];
  DataSlot view;
  int entry = -1;
  if (ds.streamed) {
    DV_TRY(stream_stage(m, ds, idx, first, B, &view, &entry));
    if (idx) idx = m->ring->iota.data();
    first = 0;
  }
  if (idx && idx_pinned) {
    memcpy(idx_pinned, idx, (size_t)B * sizeof(int));
    idx = idx_pinned;
  }
  const int st = enqueue_step(m, mode, entry >= 0 ? view : ds, idx, first, B, Bg, eps, seed);
  if (entry >= 0) {
    // also after a failed enqueue: whatever part of the step was queued may read the entry
    const int rs = stream_release(m, entry);
    if (st == OK) return rs;
  }
  return st;
}

static int run_step(dv_model* m, StepMode mode, int slot, const int32_t* idx, int64_t first, int B, int Bg,
                    const float* eps, uint64_t seed, float* out) {
  DV_TRY(check_step_args(m, slot, idx, first, B));
  if (Bg <= 0) Bg = B;
  DV_HIP(hipSetDevice(m->ctx->device));
  DV_TRY(enqueue_slot_step(m, mode, slot, idx, first, B, Bg, eps, seed));
  DV_TRY(fetch_scalars(m, Bg, out));
  return prof_flush(m);
}

// host-batch forward used by dv_infer / dv_encode
static int stage_host_batch(dv_model* m, const float* x, int nb) {
  const Arch& A = m->A;
  size_t bytes = (size_t)nb * A.H * A.H * A.C * sizeof(float);
  DV_HIP(hipMemcpyAsync(m->stage_x, x, bytes, hipMemcpyHostToDevice, m->ctx->stream));
  return OK;
}


// ---------------------------------------------------------------------------------------------------------------
// Pipelined batched inference (deblend_cutout/deblender.py:18,24: `net(tf.cast(images, tf.float32))` on all N stamps).
// The boundary hands over pageable host arrays: 83.5 KB in and 167 KB out per stamp, about what the forward pass
// itself costs in time if the copies run serially.  Chunks therefore flow through a three-stage pipeline with
// double buffers: host threads convert / copy the caller's array into pinned memory (float64 input is cast here, as
// the reference's tf.cast does) -> H2D on a copy stream -> forward on the engine streams, outputs copied device to
// device into a transfer buffer -> D2H on a second copy stream -> host threads copy into the caller's arrays.
// ---------------------------------------------------------------------------------------------------------------
struct InferPipe {
  int cap = 0;                      // stamps per buffer
  PinBuf<float> hin[2], hloc[3], hscale[3], hsmall[3];                      // pinned host (outputs: three deep)
  PinBuf<float> heps[3];            // pinned host, third image slot of the ring: Monte-Carlo std stamps (dv_infer_fields_mc_keep only)
  DevBuf<float> din[2], dloc[2], dscale[2], dsmall[2];                      // device
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_h2d[2] = {}, ev_comp[2] = {}, ev_d2h[3] = {};
  int threads = 4;
  bool host_ok = false;             // the pinned image buffers exist (calls that keep their results on the device skip them)
  ~InferPipe() {                    // (the buffers free themselves)
    for (hipEvent_t e : {ev_d2h[0], ev_d2h[1], ev_d2h[2], ev_h2d[0], ev_h2d[1], ev_comp[0], ev_comp[1]})
      if (e) (void)hipEventDestroy(e);
  }
};

static void pipe_free(InferPipe* p) { delete p; }

static int pipe_host_buffers(dv_model* m, InferPipe* p) {
  if (p->host_ok) return OK;
  const Arch& A = m->A;
  const size_t img = (size_t)p->cap * A.H * A.H * A.C;
  // a failed allocation frees what this call got so far and leaves every slot null, so that a retry on a reused pipe does
  // not keep pinned memory it cannot use (several GB at 8192 stamps per chunk)
  PinBuf<float>* slots[8] = {&p->hloc[0], &p->hscale[0], &p->hloc[1], &p->hscale[1], &p->hloc[2], &p->hscale[2], &p->hin[0], &p->hin[1]};
  for (PinBuf<float>* q : slots) {
    if (*q) continue;
    const int st = q->alloc(img, "hipHostMalloc(pinned transfer ring)");
    if (st != OK) {
      for (PinBuf<float>* r : slots) r->reset();
      return st;
    }
  }
  p->host_ok = true;
  return OK;
}

// the third image slot of the pinned ring, allocated by the first call that sends Monte-Carlo std stamps to the host
static int pipe_eps_buffers(dv_model* m, InferPipe* p) {
  const Arch& A = m->A;
  const size_t img = (size_t)p->cap * A.H * A.H * A.C;
  for (int b = 0; b < 3; ++b)
    if (!p->heps[b]) DV_TRY(p->heps[b].alloc(img, "hipHostMalloc(pinned transfer ring, epistemic slot)"));
  return OK;
}

// need_host: the call moves stamps through pinned host memory (every form except the device-resident compositing call,
// which then does not pay for ~8 GB of pinned transfer rings at 8192 stamps per chunk)
static int pipe_get(dv_model* m, int cap, InferPipe** out, bool need_host = true) {
  const Arch& A = m->A;
  if (m->pipe && m->pipe->cap >= cap) {
    if (need_host) DV_TRY(pipe_host_buffers(m, m->pipe));
    *out = m->pipe;
    return OK;
  }
  pipe_free(m->pipe);
  m->pipe = nullptr;
  std::unique_ptr<InferPipe> p(new InferPipe());
  p->cap = cap;
  const size_t img = (size_t)cap * A.H * A.H * A.C, small = (size_t)cap * 3 * A.d;   // floats (dense rows of d: the strided device rows are packed on the way)
  for (int b = 0; b < 3; ++b) {
    DV_TRY(p->hsmall[b].alloc(small));
    DV_HIP(hipEventCreateWithFlags(&p->ev_d2h[b], hipEventDisableTiming));
  }
  for (int b = 0; b < 2; ++b) {
    for (DevBuf<float>* q : {&p->din[b], &p->dloc[b], &p->dscale[b]}) DV_TRY(q->alloc(img + 16));
    DV_TRY(p->dsmall[b].alloc(small));
    DV_HIP(hipEventCreateWithFlags(&p->ev_h2d[b], hipEventDisableTiming));
    DV_HIP(hipEventCreateWithFlags(&p->ev_comp[b], hipEventDisableTiming));
  }
  p->s_in = m->ctx->red_stream;       // both idle during inference; a fifth stream would share a hardware queue
  p->s_out = m->ctx->comm_stream;
  if (need_host) DV_TRY(pipe_host_buffers(m, p.get()));
  p->threads = copy_threads();
  *out = m->pipe = p.release();
  return OK;
}

// dst[i] = (float)src[i] for n elements, split over `threads` host threads (src float32 or float64)
static void host_copy(float* dst, const void* src, size_t n, bool src_f64, int threads) {
  auto work = [=](size_t lo, size_t hi) {
    if (src_f64) {
      const double* sd = static_cast<const double*>(src);
      for (size_t i = lo; i < hi; ++i) dst[i] = (float)sd[i];
    } else {
      memcpy(dst + lo, static_cast<const float*>(src) + lo, (hi - lo) * sizeof(float));
    }
  };
  if (threads <= 1 || n < (size_t)1 << 18) {
    work(0, n);
    return;
  }
  std::vector<std::thread> pool;
  const size_t per = ((n + threads - 1) / threads + 15) & ~(size_t)15;
  for (int t = 1; t < threads; ++t) {
    const size_t lo = std::min(n, per * t), hi = std::min(n, per * (t + 1));
    if (lo < hi) pool.emplace_back(work, lo, hi);
  }
  work(0, std::min(n, per));
  for (auto& th : pool) th.join();
}

// out[i] = field[x_i : x_i + cs, y_i : y_i + cs, :] for n windows of a float64 field that lies in HOST memory, split over
// `threads` host threads: cs row copies of cs * nb doubles per window (what numpy's slice assignment does in
// extract/extraction.py:26-32).  Used for the float64 cutout_images the reference's recarray carries: the windows are exact
// copies of host data, so they are assembled on the host beside the GPU's forward passes and never cross the host link.
// sfield: the field of the stack [M][F][F][nb] each window is cut from.
static void host_gather_cutouts(double* out, const double* field, int F, int nb, const int32_t* starts, int64_t n, int cs,
                                int threads, const int32_t* sfield) {
  auto work = [=](int64_t lo, int64_t hi) {
    const size_t row = (size_t)cs * nb;
    for (int64_t i = lo; i < hi; ++i) {
      const double* src = field + (size_t)sfield[i] * F * F * nb + ((size_t)starts[2 * i] * F + starts[2 * i + 1]) * nb;
      double* dst = out + (size_t)i * cs * row;
      for (int r = 0; r < cs; ++r) memcpy(dst + r * row, src + (size_t)r * F * nb, row * sizeof(double));
    }
  };
  if (threads <= 1 || n < 64) {
    work(0, n);
    return;
  }
  std::vector<std::thread> pool;
  const int64_t per = (n + threads - 1) / threads;
  for (int t = 1; t < threads; ++t) {
    const int64_t lo = std::min(n, per * t), hi = std::min(n, per * (t + 1));
    if (lo < hi) pool.emplace_back(work, lo, hi);
  }
  work(0, std::min(n, per));
  for (auto& th : pool) th.join();
}

// stamps per chunk of an N-stamp call: the workspace capacity for long inputs, a quarter of the input (>= 128 stamps) for
// short ones
static int infer_chunk(const dv_model* m, int64_t N) {
  if (N < 2 * (int64_t)m->Bc) return (int)std::min<int64_t>(m->Bc, std::max<int64_t>(128, ((N + 3) / 4 + 63) / 64 * 64));
  return m->Bc;
}

// One run of the inference pipeline (infer_pipelined): stamps row0 .. row0 + N of the caller's list.  Every per-stamp array
// below, host or device, input or output, starts at stamp 0 of that list and is indexed by the global stamp number, as the
// Philox rows and fptr are: a caller that runs its list in several jobs (dv_infer_fields*: one per group of resident
// fields) changes row0, N, f0 and what fields_d holds between them, nothing else.  A null member is an output that is not
// wanted or a stage that does not run.
struct PipeJob {
  // source, one of two: stamps in a host array ...
  const void* x = nullptr;             // host [.][H][H][C], float32 or (x_f64) float64, cast while it is staged
  bool x_f64 = false;
  // ... or windows of float64 fields that sit in HBM, gathered and cast on the GPU (dv_infer_cutouts*, dv_infer_fields*)
  const double* fields = nullptr;      // host [M][F][F][nb]: the whole stack
  const double* fields_d = nullptr;  // device: its fields f0, f0 + 1, ...
  int F = 0, nb = 0, f0 = 0;
  const int32_t* starts = nullptr;     // host [.][2]: corner of every stamp's window
  const int* starts_d = nullptr;     // device copy of it
  const int32_t* sfield = nullptr;     // host [.]: field of every stamp
  const int* sfield_d = nullptr;     // device copy of it
  const int* fptr_d = nullptr;       // device [M + 1]: first stamp of every field
  // rows
  int64_t row0 = 0, N = 0;
  int chunk = 0;                       // stamps per chunk: infer_chunk() of the whole list
  const float* eps = nullptr;          // host [.][d] noise; null: stamp i draws Philox (seed, i)
  uint64_t seed = 0;
  // host outputs
  float *loc = nullptr, *scale = nullptr, *mu = nullptr, *zstd = nullptr, *z = nullptr;
  double* cutouts = nullptr;           // the float64 windows themselves (dv_infer_cutouts_keep), assembled on the host
  float* eps_out = nullptr;            // the Monte-Carlo std stamps (dv_infer_fields_mc_keep)
  // streaming consumer (dv_infer_cutouts_stream): reads every chunk's mean / stddev in the pinned ring, nothing is copied
  dv_chunk_fn consumer = nullptr;
  void* user = nullptr;
  // composite sums (dv_infer_cutouts_composite): every chunk's mean and stddev stamps are added into float64
  // fields in HBM right behind its forward pass instead of copied out; mean_f decides
  struct Sinks {
    double *mean_f = nullptr, *std_f = nullptr, *res_f = nullptr;   // device, fields f0 .. like fields_d
    double* eps_f = nullptr;           // the same sum of the Monte-Carlo std stamps
    double* res2_f = nullptr;          // a second residual, -= the mean stamps like res_f (dv_field_set_pass; not with eps_f)
    const int* places_d = nullptr;     // device [.][2]: field position (row, col) of every stamp's top-left corner
    double* mse = nullptr;             // device [.]: centre MSE of every stamp against its cutout
    double* eps_norm = nullptr;        // device [.]: sum(std[:, :, 2]) / sum(mean[:, :, 2]) of every stamp
  } sinks;
  // Monte-Carlo stage (dv_infer_fields_mc_*): behind every chunk's forward pass, mc_samples more decodes of
  // the encoder output that pass left in the workspace, folded into per-pixel statistics; mc_samples > 0 decides
  int mc_samples = 0;
  uint64_t mc_seed = 0;
  // position fit and fractional placements (dv_infer_fields_fit_composite): behind every chunk's forward pass
  // (and Monte-Carlo stage) the r band of its mean stamps is fitted against the resident r-band planes, the placements
  // follow from the fitted shifts on the device, and the chunk is composited there; plan decides (sinks.places_d is unused)
  struct Fit {
    const PosfitPlan* plan = nullptr;
    const int* l0 = nullptr;           // host: chunk k of the whole list runs the plan's launches l0[k] .. l0[k + 1]
    const double *img = nullptr, *totsq = nullptr;   // device: r-band planes of fields f0 .. and their sums of squares
    const double* dist_d = nullptr;    // device [.][2]: integer distances to the field centre
    double *stamps = nullptr, *work = nullptr;       // device: r band of a chunk's mean stamps, the fit's workspace
    double *shifts_d = nullptr, *obj = nullptr;      // device [.][2], [.]: start shifts in, fitted out; objective
    int *iters = nullptr, *status = nullptr;         // device [.]
    void* objs_d = nullptr;            // device [chunk]: a chunk's placements
    double* coef_d = nullptr;          // device: B-spline coefficients of a sub-chunk
  } fit;
  // catalogue measurement (dv_infer_fields_measure): behind every chunk's forward pass, fluxes and adaptive
  // moments of its mean / stddev stamps as they lie in HBM; flux decides.  Without sinks.mean_f this is the catalogue-only
  // call: no stamp and no field leaves the device
  struct Measure {
    double *flux = nullptr, *ferr = nullptr, *shape = nullptr;   // device [.][nb], [.][nb], [.][5]
    int *iters = nullptr, *status = nullptr;                     // device [.]
    int band = 0, max_iter = 0;
    double sigma0 = 0.0, tol = 0.0;
  } ms;
  // Monte-Carlo catalogue (dv_infer_fields_measure_mc): every decoder pass of the Monte-Carlo stage is measured
  // where it lies and folded into per-galaxy means and standard deviations; st.flux_mean decides (needs mc_samples > 0).  The
  // per-pixel statistics of the stage have no reader in that call and are not taken
  struct MeasureMc {
    McState st{};                      // device, rows = global stamp numbers; the running state between passes
    McScratch w{};                     // device: the rows of one decoder pass (the workspace capacity)
    int band = 0, max_iter = 0;
    double sigma0 = 0.0, tol = 0.0;
  } mcm;
  // blendedness sums (dv_infer_fields_measure_blend): behind every chunk's measurement, the child sums W, A and
  // npix of its stamps (they need the chunk's catalogue rows and sinks.places_d); blend decides.  The parent sums are the
  // caller's, once a field's composite is complete
  struct Blend {
    double* blend = nullptr;           // device [.][4]
    int* npix = nullptr;               // device [.]
  } bl;
  // the device-side mean field of a catalogue-only call whose stages read the completed composite (the blendedness sums, the
  // apertures on the fields: DESIGN.md 7l, 7p): without sinks.mean_f the chunk's mean stamps are composited into mean_f, a mean
  // field per resident field that nothing downloads; mean_f decides (needs sinks.places_d)
  struct MeanField {
    double* mean_f = nullptr;          // device, fields f0 .. like fields_d
  } mf;
  // PSF-corrected shapes (dv_infer_fields_measure_psf): behind every chunk's measurement, the re-Gaussianized
  // moments of its mean stamps from the chunk's catalogue rows and the call's PSF rows (measured before the first chunk); out
  // decides
  struct Regauss {
    const RegaussPsf* psf = nullptr;   // device: the K PSF images, their rows and residuals
    int K = 0, ps = 0;
    const int* index = nullptr;        // device [.]: PSF of every stamp
    double* out = nullptr;             // device [.][6]
    int *iters = nullptr, *status = nullptr;   // device [.]
  } rg;
  // aperture photometry (dv_infer_fields_measure_aper): behind every chunk's measurement, the circular, Kron
  // and flux-radius photometry of its mean and stddev stamps from the chunk's catalogue rows; on decides
  struct Aper {
    bool on = false;
    ApertureParams par{};
    ApertureRows rows{};               // device, row 0 = global stamp 0
  } ap;
  // the flux fit (dv_infer_fields_measure_fit) needs the mean stamps of a field once its last chunk has gone:
  // behind every chunk's measurement its mean stamps are copied into store; store decides.  The moments on the child image
  // (dv_infer_fields_measure_moments_data) read the same store: one copy of the chunk serves both
  struct FitFlux {
    float* store = nullptr;            // device [.][cs][cs][nb], row 0 = global stamp 0
  } ff;
};

// The loop of dv_infer_mc on the encoder output m->t of nb stamps: nsamples stochastic decodes, as many per pass as the
// workspace takes - the decoder runs on nb * reps rows, row r being sample k + r / nb of stamp r % nb (the sampler reads that
// stamp's t and draws the noise sample k + r / nb would get in a pass of its own: Philox (seed + sample, row0 + stamp)), and
// the per-stamp statistics fold the samples in order.  A handful of objects with 100 samples each - the per-field use of the
// reference - is one or two decoder passes instead of 100.  Leaves the mean in m->gA and the standard deviation in m->gB
// (the two gradient ping-pong buffers, unused during inference).
// mm: the per-pass hook of the Monte-Carlo catalogue - every pass is measured and folded on the main stream before the next
// pass overwrites m->loc.  pixel_stats = false (with a hook only): nothing reads the per-pixel statistics, their launches
// are left out and gA / gB keep what they held.
static int mc_decode_stats(dv_model* m, int nb, int nsamples, uint64_t seed, unsigned row0,
                           const PipeJob::MeasureMc* mm = nullptr, bool pixel_stats = true) {
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  float* mean = m->gA;
  float* m2 = m->gB;
  const int per_pass = std::max(1, m->Bc / nb);
  for (int k = 0; k < nsamples; k += per_pass) {
    const int reps = std::min(per_pass, nsamples - k);
    int nblk = 0;
    DV_TRY(sampler_forward(m, nb * reps, true, seed + (uint64_t)k, (unsigned)m->ctx->rank, row0, false, reps > 1 ? nb : 0));
    DV_TRY(decoder_forward(m, nb * reps, false));
    DV_TRY(head_lane(m, nullptr, nullptr, 0, nb * reps, nb * reps, false, true, 0, &nblk));
    // normalise=True: the recipe is np.std(deblend(net, [stamp]*100, normalise=True)[0], axis=0), i.e. the statistics
    // of the DENORMALISED means - each decoded pass goes back through sinh(arctanh(.)) before it is folded in
    if (m->normalise) DV_TRY(launch_normalise(m->loc, (long)nb * reps * stamp, true, s));
    if (mm) {
      DV_TRY(launch_measure_mc_samples(m->loc, nb * reps, A.H, A.C, mm->band, mm->sigma0, mm->tol, mm->max_iter, mm->w, s));
      DV_TRY(launch_measure_mc_fold(mm->w, nb, reps, k, nsamples, A.C, mm->st, (int64_t)row0, s));
    }
    if (!pixel_stats) continue;
    if (reps > 1)
      DV_TRY(launch_welford_update_multi(m->loc, mean, m2, (long)nb * stamp, reps, k, s));
    else
      DV_TRY(launch_welford_update(m->loc, mean, m2, ((long)(nb * stamp) + 3) & ~3L, k, s));   // buffers carry slack
  }
  if (pixel_stats) DV_TRY(launch_welford_finish(m2, ((long)(nb * stamp) + 3) & ~3L, nsamples, s));
  return OK;
}

static int infer_pipelined(dv_model* m, const PipeJob& j) {
  const Arch& A = m->A;
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  const int chunk = j.chunk, cs = A.H;
  const int64_t N = j.N, row0 = j.row0;
  const bool comp = j.sinks.mean_f != nullptr;
  const bool meas = j.ms.flux != nullptr;
  InferPipe* p = nullptr;
  DV_TRY(pipe_get(m, chunk, &p, !comp && !meas));
  if (j.eps_out) DV_TRY(pipe_eps_buffers(m, p));
  const int64_t K = (N + chunk - 1) / chunk;
  const int d = A.d;
  auto finish = [&](int64_t k) -> int {       // stage D: pinned -> caller's arrays
    const int b = (int)(k % 3);
    const int64_t r = row0 + k * chunk;       // the chunk's first stamp
    const int nb = (int)std::min<int64_t>(chunk, N - k * chunk);
    // the caller's float64 cutouts of this chunk: host work that needs nothing from the GPU, done before the wait
    if (j.cutouts)
      host_gather_cutouts(j.cutouts + r * stamp, j.fields, j.F, j.nb, j.starts + 2 * r, nb, cs, p->threads, j.sfield + r);
    DV_HIP(hipEventSynchronize(p->ev_d2h[b]));
    if (j.consumer) {
      // streaming consumer: it reads the pinned transfer buffers in place (valid until it returns), nothing is copied
      if (j.consumer(j.user, r, nb, p->hloc[b], p->hscale[b]) != 0) {
        set_error("the chunk consumer of dv_infer_cutouts_stream asked to stop at stamp %ld", (long)r);
        return E_STATE;
      }
      return OK;
    }
    if (j.loc) host_copy(j.loc + r * stamp, p->hloc[b], nb * stamp, false, p->threads);
    if (j.scale) host_copy(j.scale + r * stamp, p->hscale[b], nb * stamp, false, p->threads);
    if (j.eps_out) host_copy(j.eps_out + r * stamp, p->heps[b], nb * stamp, false, p->threads);
    if (j.mu) memcpy(j.mu + r * d, p->hsmall[b], (size_t)nb * d * sizeof(float));
    if (j.zstd) memcpy(j.zstd + r * d, p->hsmall[b] + (size_t)chunk * d, (size_t)nb * d * sizeof(float));
    if (j.z) memcpy(j.z + r * d, p->hsmall[b] + (size_t)2 * chunk * d, (size_t)nb * d * sizeof(float));
    return OK;
  };
  auto stage_in = [&](int64_t k) -> int {     // stage A, host part: caller's array -> pinned (float64 cast here)
    if (!j.x) return OK;                      // cutouts are gathered on the GPU, no host staging
    const int b = (int)(k & 1);
    const int64_t r = row0 + k * chunk;
    const int nb = (int)std::min<int64_t>(chunk, N - k * chunk);
    if (k >= 2) DV_HIP(hipEventSynchronize(p->ev_h2d[b]));            // pinned input buffer b is free again
    const char* xb = static_cast<const char*>(j.x) + (size_t)r * stamp * (j.x_f64 ? sizeof(double) : sizeof(float));
    host_copy(p->hin[b], xb, nb * stamp, j.x_f64, p->threads);
    return OK;
  };
  static const bool trace = getenv("DV_PIPE_TRACE") != nullptr;
  std::vector<hipEvent_t> tev;
  if (trace) {
    tev.resize(6 * K);
    for (auto& e : tev) DV_HIP(hipEventCreate(&e));
  }
  auto h2d = [&](int64_t k) -> int {          // stage A, device part
    const int b = (int)(k & 1);
    const int nb = (int)std::min<int64_t>(chunk, N - k * chunk);
    if (k >= 2) DV_HIP(hipStreamWaitEvent(p->s_in, p->ev_comp[b], 0));   // forward of chunk k-2 has read din[b]
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 0], p->s_in));
    if (j.x) {
      DV_HIP(hipMemcpyAsync(p->din[b], p->hin[b], nb * stamp * sizeof(float), hipMemcpyHostToDevice, p->s_in));
    } else {
      const int64_t r = row0 + k * chunk;
      DV_TRY(launch_scene_extract_f32(j.fields_d, j.F, j.nb, j.starts_d + 2 * r, nb, cs, p->din[b], p->s_in,
                                      j.sfield_d + r, j.f0));
    }
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 1], p->s_in));
    DV_HIP(hipEventRecord(p->ev_h2d[b], p->s_in));
    return OK;
  };
  if (K >= 1) {
    DV_TRY(stage_in(0));
    DV_TRY(h2d(0));
  }
  for (int64_t k = 0; k < K; ++k) {
    const int b = (int)(k & 1);
    const int64_t r = row0 + k * chunk;       // the chunk's first stamp
    const int nb = (int)std::min<int64_t>(chunk, N - k * chunk);
    // the NEXT chunk's input goes into the copy queue before this chunk's outputs: copies issued later would
    // otherwise sit behind a D2H that cannot start until this chunk's forward has finished
    if (k + 1 < K) {
      DV_TRY(stage_in(k + 1));
      DV_TRY(h2d(k + 1));
    }
    // stage B: forward, then outputs into transfer buffer b
    DV_HIP(hipStreamWaitEvent(s, p->ev_h2d[b], 0));
    if (k >= 2) DV_HIP(hipStreamWaitEvent(s, p->ev_d2h[(k - 2) % 3], 0));   // D2H of chunk k-2 has drained device buffer b
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 2], s));
    if (m->normalise) DV_TRY(launch_normalise(p->din[b], (long)nb * stamp, false, s));
    {
      // the head kernel writes loc / scale straight into transfer buffer b (a device-to-device hipMemcpyAsync of the
      // two 171 MB images cost 3.7 ms each per 2048-stamp chunk)
      float *keep_loc = m->loc, *keep_scale = m->scale;
      m->loc = p->dloc[b];
      m->scale = p->dscale[b];
      const int st = forward_all(m, p->din[b], nullptr, nullptr, 0, nb, nb, false, false, false,
                                 j.eps ? j.eps + r * d : nullptr, j.seed, (unsigned)m->ctx->rank, (unsigned)r,
                                 j.zstd != nullptr, false, true);
      m->loc = keep_loc;
      m->scale = keep_scale;
      DV_TRY(st);
    }
    if (m->normalise && (j.loc || j.consumer || comp || meas)) DV_TRY(launch_normalise(p->dloc[b], (long)nb * stamp, true, s));
    if (j.mu)
      DV_HIP(hipMemcpy2DAsync(p->dsmall[b], d * sizeof(float), m->t, A.twp * sizeof(float), d * sizeof(float), nb,
                              hipMemcpyDeviceToDevice, s));
    if (j.zstd)
      DV_TRY(copy_rows(p->dsmall[b] + (size_t)chunk * d, d, m->zstd, A.dp, d, nb, hipMemcpyDeviceToDevice, s));
    if (j.z)
      DV_TRY(copy_rows(p->dsmall[b] + (size_t)2 * chunk * d, d, m->z, A.dp, d, nb, hipMemcpyDeviceToDevice, s));
    if (j.mc_samples > 0) {
      // Monte-Carlo stage: dv_infer_mc's decodes on the encoder output the forward pass above left in m->t (no second
      // encoder pass, nothing staged from the host); sample q of stamp i draws Philox (mc seed + q, global stamp number), what
      // dv_infer_mc draws for row i of the whole stamp list.  The std stamps stay in m->gB for this chunk's sinks on the
      // output stream, so the statistics of chunk k wait until the sinks of chunk k - 1 have read theirs (they finished
      // during this chunk's forward pass).
      if (k >= 1) DV_HIP(hipStreamWaitEvent(s, p->ev_d2h[(k - 1) % 3], 0));
      LongCallKernels lk(m);             // dv_infer_mc selects kernels as a long call does, whatever N is
      if (lk.was_tiny) {
        // a call of at most 16 stamps ran its forward pass with the small-call kernels (K sliced over workgroups), whose t
        // differs from dv_infer_mc's in the last bits: encode these few stamps once more the way dv_infer_mc does
        DV_TRY(bn_prepare(m, p->din[b], nullptr, 0, nb, nb, false, false));
        DV_TRY(encoder_forward(m, p->din[b], nullptr, 0, nb, false));
      }
      const bool mcm = j.mcm.st.flux_mean != nullptr;
      DV_TRY(mc_decode_stats(m, nb, j.mc_samples, j.mc_seed, (unsigned)r, mcm ? &j.mcm : nullptr, !mcm));
    }
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 3], s));
    DV_HIP(hipEventRecord(p->ev_comp[b], s));
    // stage C: device -> pinned (three-deep ring) on the second copy stream
    const int h = (int)(k % 3);
    DV_HIP(hipStreamWaitEvent(p->s_out, p->ev_comp[b], 0));
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 4], p->s_out));
    if (comp) {
      // the consumer that follows in the reference (field_deblender.py:99-189) takes the place of the D2H stage: it runs on
      // the chunk as it lies in HBM, on the output stream, under the NEXT chunk's forward pass (an HBM-bound kernel beside
      // latency-bound ones); chunks composite in order because they share this stream, and the forward of chunk k + 2
      // waits for ev_d2h below before it overwrites the outputs this launch reads
      ProfScope ps(m, 2, p->s_out);
      // the fields this chunk's stamps belong to: one row of workgroups per field, each scanning its own objects
      const int fy0 = j.sfield[r], fy1 = j.sfield[r + nb - 1];
      if (j.fit.plan) {
        const int64_t kg = r / chunk;      // (a job starts on a chunk boundary of the whole list)
        DV_TRY(launch_posfit_band_f32(p->dloc[b], (long)nb * cs * cs, j.nb, 2, j.fit.stamps, p->s_out));
        DV_TRY(posfit_plan_run(j.fit.plan, j.fit.l0[kg], j.fit.l0[kg + 1], j.fit.img, j.fit.totsq, j.fit.stamps, j.fit.work,
                               j.fit.shifts_d, j.fit.obj, j.fit.iters, j.fit.status, p->s_out));
        DV_TRY(launch_scene_places(j.fit.dist_d + 2 * r, j.fit.shifts_d + 2 * r, nb, j.F, cs, j.fit.objs_d, p->s_out));
        DV_TRY(launch_scene_composite_frac(j.sinks.mean_f, j.sinks.std_f, j.sinks.res_f, j.F, j.nb, p->dloc[b], p->dscale[b],
                                           j.fit.objs_d, nb, cs, p->s_out, j.fptr_d, j.f0, j.sfield + r, (long)r,
                                           j.sinks.eps_f, j.sinks.eps_f ? m->gB : nullptr, j.sinks.res2_f, j.fit.coef_d));
      } else {
        DV_TRY(launch_scene_composite_chunk(j.sinks.mean_f, j.sinks.std_f, j.sinks.res_f, j.F, j.nb, p->dloc[b], p->dscale[b],
                                            j.sinks.places_d + 2 * r, nb, cs, p->s_out, j.fptr_d, j.f0, fy0, fy1 - fy0 + 1,
                                            (long)r, j.sinks.eps_f, j.sinks.eps_f ? m->gB : nullptr, j.sinks.res2_f));
      }
      if (j.sinks.eps_norm) DV_TRY(launch_scene_eps_norm(m->gB, p->dloc[b], nb, cs, j.nb, j.sinks.eps_norm + r, p->s_out));
      if (j.sinks.mse)
        DV_TRY(launch_scene_center_mse(j.fields_d, j.F, j.nb, j.starts_d + 2 * r, p->dloc[b], nb, cs, j.sinks.mse + r, p->s_out,
                                       j.sfield_d + r, j.f0));
    }
    if (meas) {
      // the catalogue of this chunk, on the output stream like the compositing: one workgroup per stamp reads the chunk's
      // mean and stddev stamps where the head kernel left them; the forward of chunk k + 2 waits for ev_d2h below
      ProfScope ps(m, 2, p->s_out);
      if (!comp && j.sinks.mse)                  // the catalogue-only call: the quality cut's input without the fields
        DV_TRY(launch_scene_center_mse(j.fields_d, j.F, j.nb, j.starts_d + 2 * r, p->dloc[b], nb, cs, j.sinks.mse + r, p->s_out,
                                       j.sfield_d + r, j.f0));
      DV_TRY(launch_measure(p->dloc[b], p->dscale[b], nb, cs, j.nb, j.ms.band, j.ms.sigma0, j.ms.tol, j.ms.max_iter,
                            j.ms.flux + (size_t)r * j.nb, j.ms.ferr + (size_t)r * j.nb, j.ms.shape + (size_t)r * 5,
                            j.ms.iters + r, j.ms.status + r, p->s_out));
      if (j.mf.mean_f && !comp)
        DV_TRY(launch_blend_composite_mean(j.mf.mean_f, j.F, j.nb, p->dloc[b], j.sinks.places_d + 2 * r, nb, cs, j.fptr_d, j.f0,
                                           j.sfield[r], j.sfield[r + nb - 1] - j.sfield[r] + 1, (long)r, p->s_out));
      if (j.bl.blend) {
        DV_TRY(launch_blend_child(p->dloc[b], j.ms.shape + (size_t)r * 5, j.ms.status + r, j.sinks.places_d + 2 * r, nb, cs,
                                  j.nb, j.ms.band, j.F, j.bl.blend + (size_t)r * 4, j.bl.npix + r, p->s_out));
      }
      if (j.rg.out)
        DV_TRY(launch_regauss(p->dloc[b], j.ms.shape + (size_t)r * 5, j.ms.status + r, j.rg.index + r, nb, cs, j.nb, j.ms.band,
                              *j.rg.psf, j.rg.K, j.rg.ps, j.ms.tol, j.ms.max_iter, j.rg.out + (size_t)r * 6, j.rg.iters + r,
                              j.rg.status + r, p->s_out));
      if (j.ap.on)
        DV_TRY(launch_aperture(p->dloc[b], p->dscale[b], j.ms.shape + (size_t)r * 5, j.ms.status + r, nb, cs, j.nb, j.ms.band,
                               j.ap.par, aperture_rows_at(j.ap.rows, r, j.ap.par, j.nb), p->s_out));
      if (j.ff.store)
        DV_HIP(hipMemcpyAsync(j.ff.store + (size_t)r * stamp, p->dloc[b], nb * stamp * sizeof(float), hipMemcpyDeviceToDevice,
                              p->s_out));
    }
    if (j.loc || j.consumer) DV_HIP(hipMemcpyAsync(p->hloc[h], p->dloc[b], nb * stamp * sizeof(float), hipMemcpyDeviceToHost, p->s_out));
    if (j.scale || j.consumer) DV_HIP(hipMemcpyAsync(p->hscale[h], p->dscale[b], nb * stamp * sizeof(float), hipMemcpyDeviceToHost, p->s_out));
    if (j.eps_out) DV_HIP(hipMemcpyAsync(p->heps[h], m->gB, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, p->s_out));
    if (j.mu || j.zstd || j.z)
      DV_HIP(hipMemcpyAsync(p->hsmall[h], p->dsmall[b], (size_t)chunk * 3 * d * sizeof(float), hipMemcpyDeviceToHost, p->s_out));
    if (trace) DV_HIP(hipEventRecord(tev[6 * k + 5], p->s_out));
    DV_HIP(hipEventRecord(p->ev_d2h[h], p->s_out));
    m->lastB = nb;
    // host work while the GPU runs: drain chunk k-2, whose D2H finished long ago - the host does not wait on the
    // GPU in steady state and the GPU always has the next forward queued.  The pinned ring slot of chunk k-2 is
    // reused by chunk k+1, which is enqueued after this drain.
    if (k >= 2) DV_TRY(finish(k - 2));
  }
  if (K >= 2) DV_TRY(finish(K - 2));
  if (K >= 1) DV_TRY(finish(K - 1));
  DV_HIP(hipStreamSynchronize(s));
  if (trace) {
    for (int64_t k = 0; k < K; ++k) {
      float t[6];
      for (int i = 0; i < 6; ++i) DV_HIP(hipEventElapsedTime(&t[i], tev[0], tev[6 * k + i]));
      fprintf(stderr, "chunk %ld: h2d %.2f-%.2f  fwd %.2f-%.2f  d2h %.2f-%.2f ms\n", (long)k, t[0], t[1], t[2], t[3], t[4], t[5]);
    }
    for (auto& e : tev) (void)hipEventDestroy(e);
  }
  return OK;
}

}  // namespace dv

// ============================================================================================
// C-ABI
// ============================================================================================
using namespace dv;

extern "C" {

int dv_version(void) { return 100; }
int dv_build_kind(void) {
#ifdef DV_DEBUG_EXPORTS
  return 1;
#else
  return 0;
#endif
}

// CRC-32C (Castagnoli), slicing-by-8 on the host: the checksum TensorFlow tensor-bundle checkpoints carry per tensor
// and per index block (debvader_amd/model/tf_checkpoint.py; reference call sites model.py:262-266, train.py:49-75).
// Same contract as tensorflow::crc32c::Extend: pass 0 (or the value returned for the preceding bytes).
uint32_t dv_crc32c(uint32_t crc, const void* data, size_t n) {
  static uint32_t tbl[8][256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      tbl[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int t = 1; t < 8; ++t) tbl[t][i] = (tbl[t - 1][i] >> 8) ^ tbl[0][tbl[t - 1][i] & 0xFF];
    init = true;
  }
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t l = crc ^ 0xFFFFFFFFu;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= l;
    l = tbl[7][lo & 0xFF] ^ tbl[6][(lo >> 8) & 0xFF] ^ tbl[5][(lo >> 16) & 0xFF] ^ tbl[4][lo >> 24] ^
        tbl[3][hi & 0xFF] ^ tbl[2][(hi >> 8) & 0xFF] ^ tbl[1][(hi >> 16) & 0xFF] ^ tbl[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n--) l = tbl[0][(l ^ *p++) & 0xFF] ^ (l >> 8);
  return l ^ 0xFFFFFFFFu;
}

int dv_last_error(char* buf, size_t n) {
  if (!buf || n == 0) return DV_E_INVALID;
  strncpy(buf, g_err, n - 1);
  buf[n - 1] = 0;
  return DV_OK;
}

int dv_config_default(dv_config* c) {
  if (!c) return DV_E_INVALID;
  memset(c, 0, sizeof *c);
  c->height = c->width = 59;
  c->bands = 6;
  c->latent_dim = 32;
  c->n_levels = 4;
  int f[4] = {32, 64, 128, 256};
  for (int i = 0; i < 4; ++i) {
    c->filters[i] = f[i];
    c->kernels[i] = 3;
  }
  c->max_batch = 256;
  c->kl_weight = 0.01f;
  c->kl_multiplicity = 2;
  c->bn_eps = 1e-3f;
  c->bn_momentum = 0.99f;
  c->bn_moving_var_unbiased = 1;
  c->sigma_floor = 1e-4f;
  c->diag_shift = 1e-5f;
  return DV_OK;
}

int dv_arch_counts(const dv_config* cfg, int32_t* n_tensors, int64_t* n_enc, int64_t* n_dec, int64_t* n_train) {
  if (!cfg) return DV_E_INVALID;
  Arch a;
  DV_TRY(a.build(cfg));
  if (n_tensors) *n_tensors = (int32_t)a.specs.size();
  if (n_enc) *n_enc = a.n_enc_params;
  if (n_dec) *n_dec = a.n_dec_params;
  if (n_train) *n_train = a.n_trainable_params;
  return DV_OK;
}

int dv_arch_describe(const dv_config* cfg, int32_t i, char* name, size_t name_len, int64_t shape[4], int32_t* ndim,
                     int32_t* trainable) {
  if (!cfg) return DV_E_INVALID;
  Arch a;
  DV_TRY(a.build(cfg));
  if (i < 0 || i >= (int)a.specs.size()) {
    set_error("tensor index %d out of range", i);
    return DV_E_INVALID;
  }
  const Spec& s = a.specs[i];
  if (name && name_len) {
    strncpy(name, s.name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (shape)
    for (int k = 0; k < 4; ++k) shape[k] = s.shape[k];
  if (ndim) *ndim = s.ndim;
  if (trainable) *trainable = s.trainable ? 1 : 0;
  return DV_OK;
}

int dv_arch_buckets(const dv_config* cfg, int64_t out[4]) {
  if (!cfg || !out) return DV_E_INVALID;
  Arch a;
  DV_TRY(a.build(cfg));
  out[0] = (int64_t)enc_bucket_split(a);
  out[1] = (int64_t)a.n_enc_train;
  out[2] = (int64_t)a.n_train;
  out[3] = (int64_t)a.n_total;
  return DV_OK;
}

int dv_arch_offset(const dv_config* cfg, int32_t i, int64_t* off, int64_t* count) {
  if (!cfg || !off || !count) return DV_E_INVALID;
  Arch a;
  DV_TRY(a.build(cfg));
  if (i < 0 || i >= (int)a.specs.size()) return DV_E_INVALID;
  *off = (int64_t)a.specs[i].off;
  *count = (int64_t)a.specs[i].count;
  return DV_OK;
}

int dv_arch_macs(const dv_config* cfg, int64_t* enc, int64_t* dec) {
  if (!cfg || !enc || !dec) return DV_E_INVALID;
  Arch a;
  DV_TRY(a.build(cfg));
  a.macs(enc, dec);
  return DV_OK;
}

int dv_device_count(int32_t* n) {
  if (!n) return DV_E_INVALID;
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    (void)hipGetLastError();
    return DV_OK;
  }
  *n = c;
  return DV_OK;
}

int dv_device_bus_id(int32_t device, char* bus_id, size_t bus_len) {
  if (!bus_id || bus_len < 16) return DV_E_INVALID;
  bus_id[0] = 0;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) {
    (void)hipGetLastError();
    set_error("dv_device_bus_id: device %d of %d visible", device, c);
    return DV_E_NODEVICE;
  }
  DV_HIP(hipDeviceGetPCIBusId(bus_id, (int)bus_len, device));
  return DV_OK;
}

// RCCL prints a five-line version banner on STDOUT when it initialises.  A process's stdout belongs to its caller
// (bench.py's contract is one JSON line there), so file descriptor 1 points at stderr while RCCL starts up.
struct StdoutToStderr {
  int saved = -1;
  StdoutToStderr() {
    fflush(stdout);
    saved = dup(1);
    if (saved >= 0 && dup2(2, 1) < 0) {
      close(saved);
      saved = -1;
    }
  }
  ~StdoutToStderr() {
    if (saved < 0) return;
    fflush(stdout);
    (void)dup2(saved, 1);
    close(saved);
  }
};

int dv_comm_unique_id(void* out_id) {
  if (!out_id) return DV_E_INVALID;
  static_assert(sizeof(ncclUniqueId) <= DV_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId id;
  {
    StdoutToStderr quiet;
    DV_NCCL(ncclGetUniqueId(&id));
  }
  memset(out_id, 0, DV_UNIQUE_ID_BYTES);
  memcpy(out_id, &id, sizeof id);
  return DV_OK;
}

// Set by an exit handler that is registered at the first dv_ctx_create, i.e. AFTER the HIP runtime registered its own:
// exit() runs handlers in reverse order, so from the moment this flag is up the runtime may already be gone and the
// destroy calls only release host memory (the process is going away; the driver reclaims the rest).  Objects whose
// destructors call the runtime (StreamRing, InferPipe, dv_field_set: DevBuf / PinBuf members, events) are NOT deleted then.
static bool g_process_exiting = false;
static void mark_process_exiting() { g_process_exiting = true; }

int dv_ctx_destroy(dv_ctx* c);
static int ctx_build(dv_ctx* c, int world, int rank, const void* unique_id) {
  DV_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  DV_HIP(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  {
    // the weight-gradient stream has slack (busy ~55 % of a step, the main stream ~96 %): lowest priority, so that its
    // kernels yield to the main stream's chain (-0.6 % on the step, three alternating same-box runs)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    DV_HIP(hipStreamCreateWithPriority(&c->aux_stream, hipStreamNonBlocking, lo));
  }
  {
    // the reduction stream's five-microsecond launches feed the bucket all-reduces and the optimizer: highest priority,
    // so that they are not queued behind whole matrix kernels (+0.3 % on the step; main / aux priorities: no effect)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    DV_HIP(hipStreamCreateWithPriority(&c->red_stream, hipStreamNonBlocking, hi));
  }
  DV_HIP(hipEventCreateWithFlags(&c->ev_red, comm_gate_event_flags()));
  // HIP multiplexes streams onto a few hardware queues (4 by default) and work on streams that share a queue runs
  // in submission order, so the engine keeps to four streams: main, comm (also the D2H stream of the inference
  // pipeline), aux, and the reduction stream (also the pipeline's H2D stream).  More forward lanes (DV_FWD_LANES > 2) create theirs on demand.
  {
    const char* wl = getenv("DV_FWD_LANES");
    const int extra = wl ? std::max(0, std::min(atoi(wl), 4) - 2) : 0;
    for (int i = 0; i < extra; ++i) DV_HIP(hipStreamCreateWithFlags(&c->lane_stream[i], hipStreamNonBlocking));
  }
  for (int i = 0; i < 3; ++i) DV_HIP(hipEventCreateWithFlags(&c->ev_lane[i], sync_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_ready, sync_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_join, comm_gate_event_flags()));
  for (int i = 0; i < 3; ++i) DV_HIP(hipEventCreateWithFlags(&c->ev_buf[i], sync_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_dec, comm_gate_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_enc, comm_gate_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_comm, sync_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_small, comm_gate_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_small2, sync_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_mid, comm_gate_event_flags()));
  DV_HIP(hipEventCreateWithFlags(&c->ev_wred, sync_event_flags()));
  DV_HIP(hipMalloc((void**)&c->red_dev, 4096 * sizeof(float)));
  if (world == 1 && getenv("DV_FORCE_COMM")) {
    // test hook: a one-rank communicator, so that the collective code paths (streams, events, in-place all-reduces)
    // run on a single-GPU box; results must equal the communicator-free path bit for bit
    ncclUniqueId id;
    StdoutToStderr quiet;
    DV_NCCL(ncclGetUniqueId(&id));
    DV_NCCL(ncclCommInitRank(&c->comm, 1, id, 0));
  }
  if (world > 1) {
    if (!unique_id) {
      set_error("world > 1 needs rank 0's unique id");
      return DV_E_INVALID;
    }
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    StdoutToStderr quiet;
#ifdef DV_DEBUG_EXPORTS
    if (getenv("DV_DEBUG_FAKE_PEERS") && atoi(getenv("DV_DEBUG_FAKE_PEERS")) != 0) {
      // rehearsal hook of the DEVELOPMENT library (see parallel.make_context): a one-rank communicator per rank, so that
      // several ranks can share the one GPU of a build box; everything else believes in `world` ranks
      fprintf(stderr, "[libdebvader_hip_debug] WARNING: DV_DEBUG_FAKE_PEERS is set: rank %d of %d gets a ONE-RANK communicator - "
                      "gradients and BN statistics are NOT summed across ranks; this is a launch rehearsal, not a job\n",
              rank, world);
      c->fake_peers = true;
      DV_NCCL(ncclGetUniqueId(&id));
      DV_NCCL(ncclCommInitRank(&c->comm, 1, id, 0));
    } else
#endif
    {
      DV_NCCL(ncclCommInitRank(&c->comm, world, id, rank));
    }
  }
  return DV_OK;
}

int dv_ctx_create(int32_t device, int32_t rank, int32_t world, const void* unique_id, dv_ctx** out) {
  if (!out || world < 1 || rank < 0 || rank >= world) {
    set_error("bad rank/world (%d/%d)", rank, world);
    return DV_E_INVALID;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    (void)hipGetLastError();
    set_error("no HIP device visible: the debvader_amd engine needs an MI355X (there is no CPU fallback)");
    return DV_E_NODEVICE;
  }
  if (device < 0 || device >= n) {
    set_error("device %d out of range (%d visible)", device, n);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(device));
  static bool exit_hook = false;
  if (!exit_hook) {
    (void)hipFree(nullptr);                 // the runtime is fully initialised (and has its exit handlers) before ours
    exit_hook = atexit(mark_process_exiting) == 0;
  }
  dv_ctx* c = new dv_ctx();
  c->device = device;
  c->rank = rank;
  c->world = world;
  g_multi_rank = world > 1;
  // every failure below releases what has been created so far (dv_ctx_destroy copes with a half-built context)
  const int st = ctx_build(c, world, rank, unique_id);
  if (st != DV_OK) {
    dv_ctx_destroy(c);
    return st;
  }
  *out = c;
  return DV_OK;
}

int dv_ctx_destroy(dv_ctx* c) {
  if (!c) return DV_OK;
  // models first: their buffers, events and pinned memory belong to this context's device and streams
  while (!c->models.empty()) dv_model_destroy(c->models.back());
  if (g_process_exiting) {
    delete c;
    return DV_OK;
  }
  (void)hipSetDevice(c->device);
  for (hipStream_t st : {c->stream, c->comm_stream, c->aux_stream, c->red_stream})
    if (st) (void)hipStreamSynchronize(st);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->red_dev) (void)hipFree(c->red_dev);
  if (c->ev_dec) (void)hipEventDestroy(c->ev_dec);
  if (c->ev_enc) (void)hipEventDestroy(c->ev_enc);
  if (c->ev_comm) (void)hipEventDestroy(c->ev_comm);
  for (auto& pr : c->cprof_comm) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (auto& pr : c->cprof_wait) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (auto e : c->cprof_pool) (void)hipEventDestroy(e);
  c->cprof_comm.clear(); c->cprof_wait.clear(); c->cprof_pool.clear();
  if (c->ev_small) (void)hipEventDestroy(c->ev_small);
  if (c->ev_small2) (void)hipEventDestroy(c->ev_small2);
  if (c->ev_mid) (void)hipEventDestroy(c->ev_mid);
  if (c->ev_wred) (void)hipEventDestroy(c->ev_wred);
  if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_red) (void)hipEventDestroy(c->ev_red);
  if (c->red_stream) (void)hipStreamDestroy(c->red_stream);
  for (int i = 0; i < 3; ++i)
    if (c->ev_buf[i]) (void)hipEventDestroy(c->ev_buf[i]);
  for (int i = 0; i < 3; ++i) {
    if (c->ev_lane[i]) (void)hipEventDestroy(c->ev_lane[i]);
    if (c->lane_stream[i]) (void)hipStreamDestroy(c->lane_stream[i]);
  }
  if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return DV_OK;
}

int dv_ctx_sync(dv_ctx* c) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipStreamSynchronize(c->stream));
  return DV_OK;
}

int dv_scene_extract(dv_ctx* c, const double* field, int32_t F, int32_t nb, const int32_t* starts, int32_t N,
                     int32_t cs, double* out) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  return scene_extract(field, F, nb, starts, N, cs, out, c->stream);
}

int dv_scene_composite(dv_ctx* c, double* field, int32_t F, int32_t nb, const double* stamps, const double* pos,
                       int32_t N, int32_t cs, double sign) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  return scene_composite(field, F, nb, stamps, pos, N, cs, sign, c->stream);
}

int dv_scene_fit_shifts(dv_ctx* c, const double* field_r, int32_t F, const double* stamps_r, int32_t N, int32_t cs,
                        const double* dist, double bound, int32_t max_iter, double* shifts_inout, double* objective,
                        int32_t* iters, int32_t* status) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  return scene_fit_shifts(field_r, F, stamps_r, N, cs, dist, bound, max_iter, shifts_inout, objective, iters, status,
                          c->stream);
}

int dv_scene_fit_shifts_fields(dv_ctx* c, const double* fields_r, int32_t M, int32_t F, const double* stamps_r,
                               const int64_t* field_ptr, int64_t N, int32_t cs, const double* dist, double bound,
                               int32_t max_iter, double* shifts_inout, double* objective, int32_t* iters, int32_t* status) {
  if (!c || N < 0 || N >= ((int64_t)1 << 31)) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  // the fields go up in groups that leave room for the fit's own buffers (up to 1.5 GiB per launch)
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t reserve = (size_t)2 << 30;
  size_t budget = free_b > reserve ? (free_b - reserve) / 10 * 8 : 0;
  if (const char* e = getenv("DV_FIELDS_GROUP_MB")) {
    const long mb = atol(e);
    if (mb > 0) budget = std::min(budget, (size_t)mb << 20);
  }
  if (budget == 0) budget = 1;                    // 0 would mean "no limit" below
  return scene_fit_shifts_fields(fields_r, M, F, stamps_r, field_ptr, (int)N, cs, dist, bound, max_iter, shifts_inout,
                                 objective, iters, status, budget, c->stream);
}

int dv_measure_params_default(dv_measure_params* p) {
  if (!p) return DV_E_INVALID;
  p->band = 2;
  p->sigma0 = 3.0;
  p->tol = 1e-10;
  p->max_iter = 200;
  return DV_OK;
}

int dv_scene_measure(dv_ctx* c, const float* mean, const float* stddev, int64_t N, int32_t cs, int32_t nb,
                     const dv_measure_params* p, double* flux, double* flux_err, double* shape, int32_t* iters,
                     int32_t* status) {
  if (!c || !p) return DV_E_INVALID;
  DV_TRY(measure_check("dv_scene_measure", cs, nb, p->band, p->sigma0, p->tol, p->max_iter));   // before any GPU work
  DV_HIP(hipSetDevice(c->device));
  return scene_measure(mean, stddev, N, cs, nb, p->band, p->sigma0, p->tol, p->max_iter,
                       CatRows{flux, flux_err, shape, iters, status}, c->stream);
}

int dv_scene_blend(dv_ctx* c, const float* stamps, const double* shape, const int32_t* status, const int32_t* places,
                   const int64_t* field_ptr, int64_t N, int32_t cs, int32_t nb, int32_t band, const double* model_fields,
                   const double* data_fields, int32_t M, int32_t F, double* blend, int32_t* npix) {
  if (!c) return DV_E_INVALID;
  DV_TRY(blend_check("dv_scene_blend", cs, nb, band));   // before any GPU work
  DV_HIP(hipSetDevice(c->device));
  return scene_blend(stamps, shape, status, places, field_ptr, N, cs, nb, band, model_fields, data_fields, M, F,
                     BlendRows{blend, npix}, c->stream);
}

int dv_scene_regauss(dv_ctx* c, const float* stamps, const double* shape, const int32_t* status, const int32_t* psf_index,
                     int64_t N, int32_t cs, int32_t nb, int32_t band, const double* psf, int32_t K, int32_t ps,
                     double psf_sigma0, double tol, int32_t max_iter, double* regauss, int32_t* regauss_iters,
                     int32_t* regauss_status, double* psf_shape, double* psf_aux, int32_t* psf_iters, int32_t* psf_status) {
  if (!c) return DV_E_INVALID;
  DV_TRY(regauss_check("dv_scene_regauss", cs, nb, band, K, ps, psf_sigma0, tol, max_iter));   // before any GPU work
  DV_HIP(hipSetDevice(c->device));
  return scene_regauss(stamps, shape, status, psf_index, N, cs, nb, band, psf, K, ps, psf_sigma0, tol, max_iter,
                       RegaussRows{regauss, regauss_iters, regauss_status}, psf_shape, psf_aux, psf_iters, psf_status, c->stream);
}

static ApertureParams aperture_params(const dv_aperture_params& a) {
  ApertureParams p{};
  p.K = a.n_radii;
  p.J = a.n_fractions;
  p.subsample = a.subsample;
  p.bisect_iters = a.bisect_iters;
  for (int k = 0; k < AP_MAX_RADII; ++k) p.radii[k] = k < a.n_radii ? a.radii[k] : 0.0;
  for (int k = 0; k < AP_MAX_FRACTIONS; ++k) p.fractions[k] = k < a.n_fractions ? a.fractions[k] : 0.0;
  p.kron_factor = a.kron_factor;
  p.kron_min = a.kron_min;
  p.kron_limit = a.kron_limit;
  return p;
}

int dv_aperture_params_default(dv_aperture_params* p) {
  if (!p) return DV_E_INVALID;
  *p = dv_aperture_params{};
  p->n_radii = 3;
  p->n_fractions = 3;
  p->subsample = 5;
  p->bisect_iters = 32;
  p->radii[0] = 3.0;
  p->radii[1] = 5.0;
  p->radii[2] = 8.0;
  p->fractions[0] = 0.2;
  p->fractions[1] = 0.5;
  p->fractions[2] = 0.8;
  p->kron_factor = 2.5;
  p->kron_min = 3.5;
  p->kron_limit = 6.0;
  return DV_OK;
}

int dv_scene_aperture(dv_ctx* c, const float* mean, const float* stddev, const double* shape, const int32_t* status, int64_t N,
                      int32_t cs, int32_t nb, int32_t band, const dv_aperture_params* params, double* ap_flux,
                      double* ap_flux_err, double* ap_area, double* flux_auto, double* flux_auto_err, double* kron,
                      double* flux_rho, int32_t* aper_flags, int32_t* aper_status) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_aperture: params must be given");
    return DV_E_INVALID;
  }
  const ApertureParams par = aperture_params(*params);
  DV_TRY(aperture_check("dv_scene_aperture", cs, nb, band, par));   // before any GPU work
  const ApertureRows out{ap_flux, ap_flux_err, ap_area, flux_auto, flux_auto_err, kron, flux_rho, aper_flags, aper_status};
  DV_HIP(hipSetDevice(c->device));
  return scene_aperture(mean, stddev, shape, status, N, cs, nb, band, par, out, c->stream);
}

int dv_scene_aperture_fields(dv_ctx* c, const double* shape, const int32_t* status, const int32_t* places,
                             const int64_t* field_ptr, const double* kron, const int32_t* aper_status, int64_t N, int32_t cs,
                             int32_t nb, const double* model_fields, const double* data_fields, int32_t M, int32_t F,
                             const dv_aperture_params* params, double* ap_model_sum, double* ap_data_sum,
                             double* ap_field_area, double* auto_model_sum, double* auto_data_sum, double* auto_field_area) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_aperture_fields: params must be given");
    return DV_E_INVALID;
  }
  const ApertureFieldRows out{ap_model_sum, ap_data_sum, ap_field_area, auto_model_sum, auto_data_sum, auto_field_area};
  // (every refusal is scene_aperture_fields')
  return scene_aperture_fields(shape, status, places, field_ptr, kron, aper_status, N, cs, nb, model_fields, data_fields, M, F,
                               aperture_params(*params), out, c->device, c->stream);
}

static_assert(DV_FIT_MAX_N == FF_MAX_N, "the header's field limit of the flux fit is the kernels'");

int dv_fit_flux_params_default(dv_fit_flux_params* p) {
  if (!p) return DV_E_INVALID;
  p->min_pivot = 1e-8;
  p->scratch_bytes = (int64_t)256 << 20;
  return DV_OK;
}

int dv_scene_fit_flux(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                      int32_t nb, const double* data_fields, int32_t M, int32_t F, const dv_fit_flux_params* params,
                      double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_fit_flux: params must be given");
    return DV_E_INVALID;
  }
  // (every refusal is scene_fit_flux's)
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes}, FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status}};
  return scene_fit_flux(stamps, places, field_ptr, N, cs, nb, data_fields, M, F, rq, c->device, c->stream);
}

// the adaptive moments on the child images D - T + P: every refusal is scene_moments_fields'
int dv_scene_moments_fields(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                            int32_t nb, const double* model_fields, const double* data_fields, const double* weight_fields,
                            int32_t M, int32_t F, const dv_measure_params* params, double* flux_data, int32_t* npix_data,
                            double* shape_data, int32_t* iters_data, int32_t* status_data) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_moments_fields: params must be given");
    return DV_E_INVALID;
  }
  return scene_moments_fields(stamps, places, field_ptr, N, cs, nb, model_fields, data_fields, weight_fields, M, F, params->band,
                              params->sigma0, params->tol, params->max_iter,
                              MomentsFieldRows{flux_data, npix_data, shape_data, iters_data, status_data}, c->device, c->stream);
}

// the same fit under per-pixel weights: every refusal is scene_fit_flux's, the null weight fields are refused here
int dv_scene_fit_flux_weighted(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N,
                               int32_t cs, int32_t nb, const double* data_fields, const double* weight_fields, int32_t M,
                               int32_t F, const dv_fit_flux_params* params, double* fit_scale, double* fit_var, double* fit_gram,
                               double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_fit_flux_weighted: params must be given");
    return DV_E_INVALID;
  }
  if (!weight_fields) {
    set_error("dv_scene_fit_flux_weighted: weight_fields must be given (dv_scene_fit_flux is the unweighted fit)");
    return DV_E_INVALID;
  }
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields};
  rq.who = "dv_scene_fit_flux_weighted";
  return scene_fit_flux(stamps, places, field_ptr, N, cs, nb, data_fields, M, F, rq, c->device, c->stream);
}

// the fit by blend groups, with weights or without: every refusal is scene_fit_flux_groups'
int dv_scene_fit_flux_groups(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                             int32_t nb, const double* data_fields, int32_t M, int32_t F, const dv_fit_flux_params* params,
                             const double* weight_fields, double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj,
                             int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, int32_t* fit_group,
                             int32_t* fit_group_size) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_fit_flux_groups: params must be given");
    return DV_E_INVALID;
  }
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields};
  rq.group = fit_group;
  rq.group_size = fit_group_size;
  rq.who = "dv_scene_fit_flux_groups";
  return scene_fit_flux_groups(stamps, places, field_ptr, N, cs, nb, data_fields, M, F, rq, c->device, c->stream);
}

int dv_scene_fit_groups(dv_ctx* c, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs, int32_t M, int32_t F,
                        int32_t* fit_group, int32_t* fit_group_size, int64_t pair_cap, int64_t* n_pairs, int32_t* pairs,
                        int64_t adj_cap, int64_t* n_adj, int32_t* adj_ptr, int32_t* adj) {
  if (!c) return DV_E_INVALID;
  return scene_fit_groups(places, field_ptr, N, cs, M, F, fit_group, fit_group_size, pair_cap, n_pairs, pairs, adj_cap, n_adj,
                          adj_ptr, adj, c->device, c->stream);
}

int dv_scene_fit_flux_gram(dv_ctx* c, const float* stamps, const int32_t* places, int64_t n, int32_t cs, int32_t nb,
                           const double* data_field, int32_t F, double* gram, double* proj) {
  if (!c) return DV_E_INVALID;
  return scene_fit_flux_gram(stamps, places, n, cs, nb, data_field, F, gram, proj, c->device, c->stream);
}

// the fit with a sky background fitted jointly, with weights or without: every refusal is scene_fit_flux's
int dv_scene_fit_flux_sky(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                          int32_t nb, const double* data_fields, const double* weight_fields, int32_t M, int32_t F,
                          const dv_fit_flux_params* params, int32_t sky_order, double* fit_scale, double* fit_var, double* fit_gram,
                          double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef,
                          double* sky_cov, int32_t* sky_status, int64_t* sky_npix) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_fit_flux_sky: params must be given");
    return DV_E_INVALID;
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "sky_npix is int64");
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields, sky_order,
                FitFluxSky{-1, sky_coef, sky_cov, sky_status, (long long*)sky_npix}};
  rq.who = "dv_scene_fit_flux_sky";
  return scene_fit_flux(stamps, places, field_ptr, N, cs, nb, data_fields, M, F, rq, c->device, c->stream);
}

// the non-negative fit, with or without weights and sky (sky_order -1: none): every refusal is scene_fit_flux's
int dv_scene_fit_flux_nonneg(dv_ctx* c, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                             int32_t nb, const double* data_fields, const double* weight_fields, int32_t M, int32_t F,
                             const dv_fit_flux_params* params, int32_t sky_order, int32_t max_iter, double* fit_scale,
                             double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status, double* fit_chi2,
                             int32_t* fit_npix, double* sky_coef, double* sky_cov, int32_t* sky_status, int64_t* sky_npix,
                             double* fit_scale_free, int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters,
                             int32_t* nonneg_status) {
  if (!c) return DV_E_INVALID;
  if (!params) {
    set_error("dv_scene_fit_flux_nonneg: params must be given");
    return DV_E_INVALID;
  }
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix, fit_scale_free, fit_clamped,
                            fit_dual},
                weight_fields, sky_order,
                FitFluxSky{sky_order == -1 ? 0 : -1, sky_coef, sky_cov, sky_status, (long long*)sky_npix},
                FitFluxNonneg{true, max_iter, nonneg_iters, nonneg_status}};
  rq.who = "dv_scene_fit_flux_nonneg";
  return scene_fit_flux(stamps, places, field_ptr, N, cs, nb, data_fields, M, F, rq, c->device, c->stream);
}

int dv_scene_fit_flux_sky_gram(dv_ctx* c, const float* stamps, const int32_t* places, int64_t n, int32_t cs, int32_t nb,
                               const double* data_field, const double* weight_field, int32_t F, int32_t sky_order, double* gram,
                               double* rhs) {
  if (!c) return DV_E_INVALID;
  return scene_fit_flux_sky_gram(stamps, places, n, cs, nb, data_field, weight_field, F, sky_order, gram, rhs, c->device, c->stream);
}

int dv_scene_measure_mc(dv_ctx* c, const float* samples, int32_t S, int64_t N, int32_t cs, int32_t nb,
                        const dv_measure_params* p, double* flux_mean, double* flux_std, double* shape_mean,
                        double* shape_std, int32_t* n_ok, double* sample_flux, double* sample_shape, int32_t* sample_status) {
  const char* who = "dv_scene_measure_mc";
  if (!c || !p) return DV_E_INVALID;
  DV_TRY(measure_check(who, cs, nb, p->band, p->sigma0, p->tol, p->max_iter));   // before any GPU work
  if (S < 1) {
    set_error("%s: %d Monte-Carlo samples given, at least 1 is needed", who, S);
    return DV_E_INVALID;
  }
  if (N < 0 || (N > 0 && (!samples || !flux_mean || !flux_std || !shape_mean || !shape_std || !n_ok))) {
    set_error("%s: samples and the Monte-Carlo outputs flux_mean, flux_std, shape_mean, shape_std and n_ok must all be given", who);
    return DV_E_INVALID;
  }
  const int given = (sample_flux != nullptr) + (sample_shape != nullptr) + (sample_status != nullptr);
  if (given != 0 && given != 3) {
    set_error("%s: the per-sample outputs sample_flux, sample_shape and sample_status go together (all given or all null)", who);
    return DV_E_INVALID;
  }
  if (N == 0) return DV_OK;
  DV_HIP(hipSetDevice(c->device));
  const McState out{flux_mean, flux_std, shape_mean, shape_std, n_ok, sample_flux, sample_shape, sample_status};
  return scene_measure_mc(samples, S, N, cs, nb, p->band, p->sigma0, p->tol, p->max_iter, out, c->stream);
}

// the C ABI's detector structs as detect.hip reads them: the weights of DESIGN 7z, the selection of 7za (the outputs only
// dv_scene_detect_multiband has stay null here) and the request of 7zb
static DetectWeights detect_weights_of(const dv_detect_weights* wt, int32_t* bad_meshes) {
  return DetectWeights{wt->weights, wt->noise, wt->filter, bad_meshes};
}
static DetectBands detect_bands_of(const dv_detect_bands* b) {
  return DetectBands{b->bands, b->k, b->band_weights, b->planes, b->planes != nullptr, b->noise, b->filter};
}
static DetectObjects detect_objects_of(const dv_detect_objects* o) {
  return DetectObjects{{o->xmin, o->xmax, o->ymin, o->ymax, o->xpeak, o->ypeak, o->xvpeak, o->yvpeak, o->flag},
                       {o->vpeak, o->dflux, o->x_iso, o->y_iso, o->x2, o->y2, o->xy},
                       o->segmap};
}

int dv_scene_detect(dv_ctx* c, const double* fields, int32_t M, int32_t H, int32_t W, const dv_detect_params* p,
                    int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms, int32_t* field, int32_t* parent,
                    int32_t* npix, double* peak, double* flux, double* x, double* y, double* back, double* rms,
                    double* D, int32_t* labels) {
  if (!c || !p) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  DetectRequest rq{fields, 0, M, H, W, p};
  rq.back_h = back; rq.rms_h = rms; rq.D_h = D; rq.labels_h = labels;
  rq.cat = DetectCatalog{cap, n_out, offsets, globalrms, field, parent, npix, peak, flux, x, y};
  return scene_detect(rq, c->stream);
}

int dv_scene_detect_weighted(dv_ctx* c, const double* fields, int32_t M, int32_t H, int32_t W, const dv_detect_params* p,
                             int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms, int32_t* field,
                             int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y, double* back,
                             double* rms, double* D, int32_t* labels, const dv_detect_weights* wt, int32_t* bad_meshes) {
  if (!c || !p) return DV_E_INVALID;
  if (!wt || !wt->weights) {
    set_error("dv_scene_detect_weighted: the weights must be given (dv_scene_detect is the call without them)");
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(c->device));
  const DetectWeights wq = detect_weights_of(wt, bad_meshes);
  DetectRequest rq{fields, 0, M, H, W, p};
  rq.weights = &wq;
  rq.back_h = back; rq.rms_h = rms; rq.D_h = D; rq.labels_h = labels;
  rq.cat = DetectCatalog{cap, n_out, offsets, globalrms, field, parent, npix, peak, flux, x, y};
  return scene_detect(rq, c->stream);
}

int dv_scene_detect_multiband(dv_ctx* c, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                              const dv_detect_params* p, int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms,
                              int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y,
                              double* back, double* rms, double* V, double* Wt, double* D, int32_t* labels,
                              const dv_detect_bands* b, double* band_globalrms, int32_t* bad_meshes) {
  if (!c || !p) return DV_E_INVALID;
  if (!b) {
    set_error("dv_scene_detect_multiband: the band selection must be given");
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(c->device));
  if (!fields) {
    set_error("scene_detect_multiband: bad arguments");
    return DV_E_INVALID;
  }
  DetectBands mb = detect_bands_of(b);
  mb.band_grms_h = band_globalrms; mb.bad_meshes_h = bad_meshes; mb.V_h = V; mb.Wt_h = Wt;
  DetectRequest rq{fields, nb, M, H, W, p};
  rq.bands = &mb;
  rq.back_h = back; rq.rms_h = rms; rq.D_h = D; rq.labels_h = labels;
  rq.cat = DetectCatalog{cap, n_out, offsets, globalrms, field, parent, npix, peak, flux, x, y};
  return scene_detect(rq, c->stream);
}

int dv_scene_detect_objects(dv_ctx* c, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                            const dv_detect_params* p, int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms,
                            int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y,
                            const dv_detect_weights* wt, const dv_detect_bands* b, const dv_detect_objects* objects) {
  if (!c || !p) return DV_E_INVALID;
  if (!objects) {
    set_error("dv_scene_detect_objects: the objects request must be given (the other detect calls are the ones without it)");
    return DV_E_INVALID;
  }
  if (wt && b) {
    set_error("dv_scene_detect_objects: single-band weights and a band selection exclude each other");
    return DV_E_INVALID;
  }
  if (wt && !wt->weights) {
    set_error("dv_scene_detect_objects: a weights struct without weights");
    return DV_E_INVALID;
  }
  if (p->thresh < 0.0) {
    set_error("dv_scene_detect_objects: thresh must be >= 0, the moments' weights are the pixels above it (got %g)", p->thresh);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(c->device));
  if (!fields || (!b && nb != 0)) {
    set_error("scene_detect_objects: bad arguments (fields [M][H][W] with nb = 0, or [M][H][W][nb] with a band selection and "
              "no single-band weights)");
    return DV_E_INVALID;
  }
  const DetectObjects oq = detect_objects_of(objects);
  DetectWeights wq{};
  if (wt) wq = detect_weights_of(wt, nullptr);
  DetectBands mb{};
  if (b) mb = detect_bands_of(b);
  DetectRequest rq{fields, nb, M, H, W, p};
  rq.weights = wt ? &wq : nullptr; rq.bands = b ? &mb : nullptr; rq.objects = &oq;
  rq.cat = DetectCatalog{cap, n_out, offsets, globalrms, field, parent, npix, peak, flux, x, y};
  return scene_detect(rq, c->stream);
}

// (7zc) the refusals of a cleaning request that need no field: a null struct, clean_param, thresh, minarea
static int detect_clean_check(const char* who, bool given, double clean_param, const dv_detect_params* p) {
  if (!given) {
    set_error("%s: the clean request must be given (dv_scene_detect_objects is the call without it)", who);
    return DV_E_INVALID;
  }
  if (!std::isfinite(clean_param) || !(clean_param > 0.0)) {
    set_error("%s: clean_param must be finite and > 0 (got %g)", who, clean_param);
    return DV_E_INVALID;
  }
  if (!(p->thresh > 0.0)) {
    set_error("%s: the cleaning pass compares profiles with the threshold, thresh must be > 0 (got %g)", who, p->thresh);
    return DV_E_INVALID;
  }
  if (p->minarea > 64) {
    set_error("%s: the cleaning pass takes minarea up to 64 (got %d)", who, p->minarea);
    return DV_E_INVALID;
  }
  return DV_OK;
}

int dv_scene_detect_clean(dv_ctx* c, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                          const dv_detect_params* p, int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms,
                          int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y,
                          const dv_detect_weights* wt, const dv_detect_bands* b, const dv_detect_objects* objects,
                          const dv_detect_clean* clean) {
  if (!c || !p) return DV_E_INVALID;
  if (wt && b) {
    set_error("dv_scene_detect_clean: single-band weights and a band selection exclude each other");
    return DV_E_INVALID;
  }
  if (wt && !wt->weights) {
    set_error("dv_scene_detect_clean: a weights struct without weights");
    return DV_E_INVALID;
  }
  DV_TRY(detect_clean_check("dv_scene_detect_clean", clean != nullptr, clean ? clean->clean_param : 0.0, p));
  DV_HIP(hipSetDevice(c->device));
  if (!fields || (!b && nb != 0)) {
    set_error("scene_detect_clean: bad arguments (fields [M][H][W] with nb = 0, or [M][H][W][nb] with a band selection and "
              "no single-band weights)");
    return DV_E_INVALID;
  }
  DetectObjects oq{};
  if (objects) oq = detect_objects_of(objects);
  DetectWeights wq{};
  if (wt) wq = detect_weights_of(wt, nullptr);
  DetectBands mb{};
  if (b) mb = detect_bands_of(b);
  const DetectClean cq{clean->clean_param, clean->nmerged, clean->mthresh, clean->n_raw};
  DetectRequest rq{fields, nb, M, H, W, p};
  rq.weights = wt ? &wq : nullptr; rq.bands = b ? &mb : nullptr; rq.objects = objects ? &oq : nullptr; rq.clean = &cq;
  rq.cat = DetectCatalog{cap, n_out, offsets, globalrms, field, parent, npix, peak, flux, x, y};
  return scene_detect(rq, c->stream);
}

int dv_ctx_allreduce_host(dv_ctx* c, float* buf, int32_t n) {
  if (!c || !buf || n < 0 || n > 4096) return DV_E_INVALID;
  if (!c->comm || n == 0) return DV_OK;
  DV_HIP(hipMemcpyAsync(c->red_dev, buf, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  DV_TRY(allreduce_small(c, c->red_dev, (size_t)n));
  DV_HIP(hipMemcpyAsync(buf, c->red_dev, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  DV_HIP(hipStreamSynchronize(c->stream));
  return DV_OK;
}

int dv_model_destroy(dv_model* m) {
  if (!m) return DV_OK;
  if (m->ctx) {
    auto& v = m->ctx->models;
    v.erase(std::remove(v.begin(), v.end(), m), v.end());
  }
  if (g_process_exiting) {
    // see mark_process_exiting: host memory only.  The ring, the pipeline and the field sets own device and pinned memory,
    // events and a stream, which their destructors would hand back to a runtime that may be gone: they are left behind
    delete m;
    return DV_OK;
  }
  (void)hipSetDevice(m->ctx->device);
  // every stream a step or an inference call may have queued work on (weight gradients, reductions, collectives)
  for (hipStream_t st : {m->ctx->stream, m->ctx->aux_stream, m->ctx->red_stream, m->ctx->comm_stream})
    if (st) (void)hipStreamSynchronize(st);
  for (hipStream_t st : m->ctx->lane_stream)
    if (st) (void)hipStreamSynchronize(st);
  for (void* p : m->allocs) (void)hipFree(p);
  for (int s = 0; s < 2; ++s) {
    if (m->slots[s].x) (void)hipFree(m->slots[s].x);
    if (m->slots[s].y) (void)hipFree(m->slots[s].y);
  }
  if (m->ring && m->ring->copy) (void)hipStreamSynchronize(m->ring->copy);
  ring_free(m);
  pipe_free(m->pipe);
  for (dv_field_set* fs : m->field_sets) {
    field_set_release(fs);
    delete fs;
  }
  for (auto& kv : m->infer_graphs) (void)hipGraphExecDestroy(kv.second);
  for (int k = 0; k < 3; ++k) {
    if (m->ev_wk[k]) (void)hipEventDestroy(m->ev_wk[k]);
    if (m->ev_rk[k]) (void)hipEventDestroy(m->ev_rk[k]);
  }
  if (m->ev_bnpre) (void)hipEventDestroy(m->ev_bnpre);
  if (m->ev_bnpre_go) (void)hipEventDestroy(m->ev_bnpre_go);
  (void)hipHostFree(m->ring_scal);
  (void)hipHostFree(m->ring_idx);
  for (auto& e : m->ring_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto e : m->ev_pool) (void)hipEventDestroy(e);
  for (auto& r : m->prof) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  delete m;
  return DV_OK;
}

int dv_model_create(dv_ctx* ctx, const dv_config* cfg, dv_model** out) {
  if (!ctx || !cfg || !out) return DV_E_INVALID;
  if (cfg->max_batch < 1) {
    set_error("max_batch must be >= 1");
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(ctx->device));
  dv_model* m = new dv_model();
  m->ctx = ctx;
  int st = m->A.build(cfg);
  if (st != OK) {
    delete m;
    return st;
  }
  ctx->models.push_back(m);
  const Arch& A = m->A;
  const size_t Bc = (size_t)cfg->max_batch;
  m->Bc = cfg->max_batch;
  m->infer_graph = cfg->infer_graph != 0;
  if (cfg->dtype == DV_DTYPE_F32) {
    // The fp32 weight-gradient and tiled kernels address a layer's tensors with 32-bit ELEMENT offsets.  A training step
    // has no lanes, so a max_batch whose largest activation reaches 2^31 elements would fail inside the first step, with
    // half of it queued (and, with several ranks, peers left inside collectives): refuse it here.
    size_t per_stamp = (size_t)A.H * A.H * A.C0p;
    for (int j = 0; j < 2 * A.L; ++j) {
      int hin, cin, hout, cout, s;
      A.enc_layer(j, &hin, &cin, &hout, &cout, &s);
      per_stamp = std::max(per_stamp, (size_t)hout * hout * cout);
      A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
      per_stamp = std::max(per_stamp, (size_t)hout * hout * cout);
    }
    per_stamp = std::max(per_stamp, (size_t)A.dec_out * A.dec_out * A.C2p);
    per_stamp = std::max(per_stamp, (size_t)A.twp);   // the rows of t and d(t): the largest at a wide latent_dim
    if (Bc * per_stamp >= ((size_t)1 << 31)) {
      set_error("max_batch %d x %zu elements of the largest activation reaches 2^31: the fp32 engine addresses a layer with "
                "32-bit element offsets; use max_batch <= %zu (inference splits larger inputs into chunks by itself)",
                cfg->max_batch, per_stamp, (((size_t)1 << 31) - 1) / per_stamp);
      return dv_model_destroy(m), DV_E_INVALID;
    }
  }
  if (cfg->dtype != DV_DTYPE_F32 && cfg->dtype != DV_DTYPE_BF16) {
    set_error("unknown dtype %d", cfg->dtype);
    return dv_model_destroy(m), DV_E_INVALID;
  }
  const bool bf16 = cfg->dtype == DV_DTYPE_BF16;
  if (bf16 && Bc * A.twp >= ((size_t)1 << 31)) {
    // (the trunk kernels address the t / d(t) rows and their K-split slabs with 64-bit offsets, but the Dense layers of
    // the engine's fallback path take 32-bit element offsets)
    set_error("max_batch %d x %d elements of the t / d(t) rows reaches 2^31: the Dense layers address a tensor with 32-bit "
              "element offsets; use max_batch <= %zu", cfg->max_batch, A.twp, (((size_t)1 << 31) - 1) / A.twp);
    return dv_model_destroy(m), DV_E_INVALID;
  }
  const size_t Ba = bf16 ? 0 : Bc;   // fp32 activations of the conv stacks: not allocated by the bf16 engine
  size_t max_act = 0;  // largest per-stamp activation (elements) for the gradient ping-pong buffers
  auto track = [&](size_t e) { max_act = std::max(max_act, e); };
  auto fail = [&](int s) {
    dv_model_destroy(m);
    return s;
  };
#define ALLOC(ptr, elems)                         \
  do {                                            \
    int s__ = dalloc(m, &(ptr), (size_t)(elems)); \
    if (s__ != OK) return fail(s__);              \
  } while (0)
  ALLOC(m->P, A.n_total);
  ALLOC(m->G, A.n_total);
  ALLOC(m->Mm, A.n_total);
  ALLOC(m->Vv, A.n_total);
  const size_t k0sq = (size_t)cfg->kernels[0] * cfg->kernels[0];
  ALLOC(m->W1p, k0sq * A.C0p * cfg->filters[0]);
  ALLOC(m->G0s, k0sq * A.C0p * cfg->filters[0]);
  ALLOC(m->Whp, 9 * cfg->filters[0] * A.C2p);
  ALLOC(m->Ghs, 9 * cfg->filters[0] * A.C2p);
  ALLOC(m->bhp, A.C2p);
  size_t in_e = (size_t)A.H * A.H * A.C0p;
  ALLOC(m->xn, Ba * in_e);
  track(in_e);
  ALLOC(m->stage_x, Bc * A.H * A.H * A.C);
  m->enc_u.resize(2 * A.L);
  m->enc_a.resize(2 * A.L);
  m->dec_u.resize(2 * A.L);
  m->dec_a.resize(2 * A.L);
  m->du_enc.assign(2 * A.L, nullptr);
  m->du_dec.assign(2 * A.L, nullptr);
  for (int j = 0; j < 2 * A.L; ++j) {
    int hin, cin, hout, cout, s;
    A.enc_layer(j, &hin, &cin, &hout, &cout, &s);
    size_t e = (size_t)hout * hout * cout;
    ALLOC(m->enc_u[j], Ba * e);
    ALLOC(m->enc_a[j], Ba * e);
    if (!bf16) track(e);
  }
  track(A.flat);
  ALLOC(m->flat_a, Bc * A.flat);
  ALLOC(m->t, Bc * A.twp);
  track(A.twp);
  ALLOC(m->eps, Bc * A.dp);
  ALLOC(m->z, Bc * A.dp);
  ALLOC(m->zstd, Bc * A.dp);
  if (A.twp != A.tw) {
    ALLOC(m->Wdp, (size_t)A.flat * A.twp);
    ALLOC(m->Gdp, (size_t)A.flat * A.twp);
    ALLOC(m->bdp, A.twp);
  }
  if (A.dp != A.d) {
    ALLOC(m->W0p, (size_t)A.dp * A.dec_hidden);
    ALLOC(m->G0p, (size_t)A.dp * A.dec_hidden);
  }
  ALLOC(m->kl, Bc);
  ALLOC(m->dec_ain, Bc * A.dp);
  ALLOC(m->dec_uh, Bc * A.dec_hidden);
  ALLOC(m->dec_ah, Bc * A.dec_hidden);
  size_t r = (size_t)A.w0 * A.w0 * cfg->filters[A.L - 1];
  ALLOC(m->dec_ur, Bc * r);
  ALLOC(m->dec_ar, Bc * r);
  track(r);
  track(A.dec_hidden);
  for (int j = 0; j < 2 * A.L; ++j) {
    int hin, cin, hout, cout, s;
    A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
    size_t e = (size_t)hout * hout * cout;
    ALLOC(m->dec_u[j], Ba * e);
    ALLOC(m->dec_a[j], Ba * e);
    if (!bf16) track(e);
  }
  size_t head_e = (size_t)A.dec_out * A.dec_out * A.C2p;
  ALLOC(m->tpre, Ba * head_e);
  if (!bf16) track(head_e);
  ALLOC(m->loc, Bc * A.H * A.H * A.C + 4);
  ALLOC(m->scale, Bc * A.H * A.H * A.C + 4);
  ALLOC(m->gA, Bc * max_act);
  ALLOC(m->gB, Bc * max_act);
  ALLOC(m->gC, Bc * max_act);
  {
    float* sd = nullptr;
    ALLOC(sd, 4);
    m->seed_dev = reinterpret_cast<unsigned long long*>(sd);
  }
  m->gbufs = {m->gA, m->gB, m->gC};
  m->max_act_elems = Bc * max_act;
  // workspaces: ws1 weight-gradient slabs, ws2 d(alpha) partials, ws3 small reductions
  size_t max_w = 0;
  for (auto& s : A.specs)
    if (s.ndim >= 2) max_w = std::max(max_w, s.count);
  max_w = std::max(max_w, k0sq * A.C0p * cfg->filters[0]);
  m->ws1_elems = std::max((size_t)32 << 20, (max_w + 1024) * 3);   // three rotating regions, each at least one slab
  ALLOC(m->ws1, m->ws1_elems);
  m->ws4_elems = (size_t)4 * 16 * Bc * std::max((size_t)A.flat, (size_t)A.tw);
  ALLOC(m->ws4, m->ws4_elems);
  m->wstream = ctx->stream;
  if (getenv("DV_NO_OVERLAP")) m->overlap_wgrad = false;
  if (getenv("DV_NO_FWD_SPLIT")) m->split_forward = false;
  if (g_fuse_prelu_bwd) m->no_fuse = false;
  m->arena_elems = 0;
  for (auto& sp : A.specs)
    if (sp.name.size() > 6 && sp.name.compare(sp.name.size() - 6, 6, "/alpha") == 0)
      m->arena_elems += (size_t)std::max<size_t>(33, bf16 ? 2 * ((Bc + 63) / 64) + 2 : 0) * ((sp.count + 3) & ~(size_t)3) + 65536;
  ALLOC(m->arena, m->arena_elems);
  m->ws2_elems = std::max((size_t)1 << 20, max_act * 16);
  ALLOC(m->ws2, m->ws2_elems);
  size_t head_blocks = (Bc * A.dec_out * A.dec_out + 255) / 256;
  m->ws3_elems = std::max((size_t)1 << 20, head_blocks * 2 + 64);
  m->ws3_elems = std::max(m->ws3_elems, (size_t)64 * std::max((size_t)A.flat, r));
  // the encoder Dense bias gradient's column partials (bias_grad_colsum over the rows of d(t)): wide at a large latent_dim
  m->ws3_elems = std::max(m->ws3_elems, (std::max<size_t>((Bc + 2047) / 2048, 64) + 1) * A.twp);
  // BN statistics / BN backward partials: one 16-float row per 1024 pixels of the batch (the capacity used to
  // be derived from other users of the buffer and overran silently above ~19k stamps of 59 px)
  m->ws3_elems = std::max(m->ws3_elems, ((Bc * (size_t)A.H * A.H + 1023) / 1024 + 1) * (2 * DV_BN_MAXC));
  ALLOC(m->ws3, m->ws3_elems);
  if (bf16) ALLOC(m->ws_head, m->ws3_elems);
  ALLOC(m->scal, 16);
  ALLOC(m->zero_page, 64);
  ALLOC(m->bnstate, 4 * DV_BN_MAXC);
  ALLOC(m->bnsums, 2 * DV_BN_MAXC);
  ALLOC(m->bn_pre_sums, 2 * DV_BN_MAXC);
  m->bn_pre_part_elems = (size_t)(2 * DV_BN_MAXC) * (((size_t)Bc * A.H * A.H + 1023) / 1024 + 16);
  ALLOC(m->bn_pre_part, m->bn_pre_part_elems);
  for (int k = 0; k < 3; ++k)
    if (hipEventCreateWithFlags(&m->ev_wk[k], sync_event_flags()) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_rk[k], sync_event_flags()) != hipSuccess)
      return fail(E_HIP);
  if (hipEventCreateWithFlags(&m->ev_bnpre, sync_event_flags()) != hipSuccess ||
      hipEventCreateWithFlags(&m->ev_bnpre_go, comm_gate_event_flags()) != hipSuccess)
    return fail(E_HIP);
  {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, Bc * sizeof(int));
    if (e != hipSuccess) return fail(hip_fail(e, "hipMalloc", __FILE__, __LINE__));
    m->allocs.push_back(q);
    m->idx_dev = (int*)q;
    q = nullptr;
    e = hipMalloc(&q, (size_t)4 * Bc * sizeof(int));
    if (e != hipSuccess) return fail(hip_fail(e, "hipMalloc", __FILE__, __LINE__));
    m->allocs.push_back(q);
    m->idx_slots = (int*)q;
  }
#undef ALLOC
  hipStream_t s = ctx->stream;
  if (hipMemsetAsync(m->P, 0, A.n_total * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->G, 0, A.n_total * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->Mm, 0, A.n_total * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->Vv, 0, A.n_total * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->scal, 0, 16 * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->zero_page, 0, 64 * sizeof(float), s) != hipSuccess ||
      hipMemsetAsync(m->bnsums, 0, 2 * DV_BN_MAXC * sizeof(float), s) != hipSuccess)
    return fail(E_HIP);
  if (A.dp != A.d || A.twp != A.tw) {                // pad columns of the latent-sized rows: zero from the start
    if (hipMemsetAsync(m->eps, 0, Bc * A.dp * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(m->z, 0, Bc * A.dp * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(m->zstd, 0, Bc * A.dp * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(m->dec_ain, 0, Bc * A.dp * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(m->t, 0, Bc * A.twp * sizeof(float), s) != hipSuccess)
      return fail(E_HIP);
  }
  if (bf16) {
    st = bf_alloc(m);
    if (st != OK) return fail(st);
  } else if (m->use_wino) {
    // Winograd-domain weights of every stride-1 3x3 layer, forward and data-gradient form (wino.hip)
    auto reg = [&](const float* W, bool nmajor, const Taps& tp, int cin, int cout) -> int {
      if (!wino_supported(1, 8, cin, cout) || tp.n != 9) return OK;
      return wino_register(m, W, nmajor, tp, cin, cout, nullptr);
    };
    const Taps tf = taps_fprop(1), td = taps_dgrad(1, 1, 0, 0);
    for (int j = 0; j < 2 * A.L && st == OK; ++j) {
      int hin, cin, hout, cout, sd;
      A.enc_layer(j, &hin, &cin, &hout, &cout, &sd);
      if (sd == 1 && j > 0) {
        st = reg(m->P + A.specs[A.enc_k(j)].off, false, tf, cin, cout);
        if (st == OK) st = reg(m->P + A.specs[A.enc_k(j)].off, true, td, cout, cin);
      }
      A.dec_layer(j, &hin, &cin, &hout, &cout, &sd);
      if (sd == 1 && st == OK) {
        st = reg(m->P + A.specs[A.dec_k(j)].off, true, td, cin, cout);
        if (st == OK) st = reg(m->P + A.specs[A.dec_k(j)].off, false, tf, cout, cin);
      }
    }
    if (st == OK) st = reg(m->Whp, false, tf, cfg->filters[0], A.C2p);
    if (st == OK) st = reg(m->Whp, true, td, A.C2p, cfg->filters[0]);
    if (st == OK && !m->wino.empty()) st = wino_upload_descs(m, ctx->stream);
    if (st != OK) return fail(st);
  }
  st = dv_model_init(m, 0);
  if (st != OK) return fail(st);
  *out = m;
  return DV_OK;
}

// host-side Philox for the Glorot draws
static void philox_host(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t c[4] = {c0, c1, 0x243F6A88u, 0x85A308D3u};
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  for (int i = 0; i < 4; ++i) out[i] = c[i];
}

int dv_model_init(dv_model* m, uint64_t seed) {
  if (!m) return DV_E_INVALID;
  const Arch& A = m->A;
  DV_HIP(hipSetDevice(m->ctx->device));
  std::vector<float> h(A.n_total, 0.f);
  for (size_t i = 0; i < A.specs.size(); ++i) {
    const Spec& s = A.specs[i];
    const std::string& n = s.name;
    auto ends = [&](const char* suf) {
      size_t l = strlen(suf);
      return n.size() >= l && n.compare(n.size() - l, l, suf) == 0;
    };
    float* dst = h.data() + s.off;
    if (ends("/kernel")) {
      double fan_in, fan_out;
      if (s.ndim == 4) {
        fan_in = (double)s.shape[0] * s.shape[1] * s.shape[2];
        fan_out = (double)s.shape[0] * s.shape[1] * s.shape[3];
      } else {
        fan_in = (double)s.shape[0];
        fan_out = (double)s.shape[1];
      }
      double lim = sqrt(6.0 / (fan_in + fan_out));  // Keras glorot_uniform
      for (size_t e = 0; e < s.count; e += 4) {
        uint32_t r[4];
        philox_host((uint32_t)(e / 4), (uint32_t)i, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        for (int k = 0; k < 4 && e + k < s.count; ++k)
          dst[e + k] = (float)((((double)r[k] + 0.5) / 4294967296.0 * 2.0 - 1.0) * lim);
      }
    } else if (ends("/gamma") || ends("/moving_variance")) {
      for (size_t e = 0; e < s.count; ++e) dst[e] = 1.f;
    }
  }
  DV_HIP(hipMemcpyAsync(m->P, h.data(), A.n_total * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  DV_TRY(refresh_w1p(m));
  DV_TRY(refresh_head_pad(m));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  return DV_OK;
}

static int tensor_io(dv_model* m, float* base, int32_t i, float* host, size_t nbytes, bool to_host) {
  if (!m || !host) return DV_E_INVALID;
  const Arch& A = m->A;
  if (i < 0 || i >= (int)A.specs.size()) {
    set_error("tensor index %d out of range", i);
    return DV_E_INVALID;
  }
  const Spec& s = A.specs[i];
  if (nbytes != s.count * sizeof(float)) {
    set_error("tensor %s holds %zu bytes, caller passed %zu", s.name.c_str(), s.count * sizeof(float), nbytes);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(m->ctx->device));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  if (to_host)
    DV_HIP(hipMemcpy(host, base + s.off, nbytes, hipMemcpyDeviceToHost));
  else
    DV_HIP(hipMemcpy(base + s.off, host, nbytes, hipMemcpyHostToDevice));
  return DV_OK;
}

int dv_model_get_param(dv_model* m, int32_t i, float* host, size_t nbytes) {
  return tensor_io(m, m ? m->P : nullptr, i, host, nbytes, true);
}
int dv_model_set_param(dv_model* m, int32_t i, const float* host, size_t nbytes) {
  DV_TRY(tensor_io(m, m ? m->P : nullptr, i, const_cast<float*>(host), nbytes, false));
  m->bf.dirty_mask = 7;
  m->param_epoch++;
  if (i == m->A.head_k() || i == m->A.head_b()) {
    DV_TRY(refresh_head_pad(m));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
  }
  if (i == m->A.D0 + 1 && m->W0p) {
    DV_TRY(refresh_head_pad(m));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
  }
  if (i == m->A.enc_k(0) || i == 0 || i == 1 || ((i == m->A.enc_dk() || i == m->A.enc_db()) && m->Wdp)) {
    DV_TRY(refresh_w1p(m));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
  }
  return DV_OK;
}
int dv_model_get_grad(dv_model* m, int32_t i, float* host, size_t nbytes) {
  return tensor_io(m, m ? m->G : nullptr, i, host, nbytes, true);
}
int dv_model_get_slot(dv_model* m, int32_t i, int32_t which, float* host, size_t nbytes) {
  if (!m || which < 0 || which > 1) return DV_E_INVALID;
  return tensor_io(m, which == 0 ? m->Mm : m->Vv, i, host, nbytes, true);
}
int dv_model_set_slot(dv_model* m, int32_t i, int32_t which, const float* host, size_t nbytes) {
  if (!m || which < 0 || which > 1) return DV_E_INVALID;
  return tensor_io(m, which == 0 ? m->Mm : m->Vv, i, const_cast<float*>(host), nbytes, false);
}

int dv_model_set_trainable(dv_model* m, int32_t enc, int32_t dec) {
  if (!m) return DV_E_INVALID;
  m->enc_trainable = enc != 0;
  m->dec_trainable = dec != 0;
  return DV_OK;
}

int dv_optimizer_reset(dv_model* m, float lr, float b1, float b2, float eps) {
  if (!m) return DV_E_INVALID;
  DV_HIP(hipSetDevice(m->ctx->device));
  m->lr = lr;
  m->b1 = b1;
  m->b2 = b2;
  m->aeps = eps;
  m->iter = 0;
  m->opt_enc = m->enc_trainable;
  m->opt_dec = m->dec_trainable;
  DV_HIP(hipMemsetAsync(m->Mm, 0, m->A.n_total * sizeof(float), m->ctx->stream));
  DV_HIP(hipMemsetAsync(m->Vv, 0, m->A.n_total * sizeof(float), m->ctx->stream));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  return DV_OK;
}
int dv_optimizer_get_iter(dv_model* m, int64_t* it) {
  if (!m || !it) return DV_E_INVALID;
  *it = m->iter;
  return DV_OK;
}
int dv_optimizer_set_iter(dv_model* m, int64_t it) {
  if (!m || it < 0) return DV_E_INVALID;
  m->iter = it;
  return DV_OK;
}

int dv_data_free(dv_model* m, int32_t slot) {
  if (!m || slot < 0 || slot > 1) return DV_E_INVALID;
  DV_HIP(hipSetDevice(m->ctx->device));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  if (m->slots[slot].x) (void)hipFree(m->slots[slot].x);
  if (m->slots[slot].y) (void)hipFree(m->slots[slot].y);
  m->slots[slot] = DataSlot();
  if (m->ring && !m->slots[0].streamed && !m->slots[1].streamed) {
    // no slot streams any more: the ring goes once nothing queued can still read or write it
    DV_TRY(ring_sync_streams(m));
    ring_free(m);
  }
  return DV_OK;
}

int dv_data_stream_open(dv_model* m, int32_t slot, const void* x, int32_t x_f64, const void* y, int32_t y_f64, int64_t n,
                        int64_t row_stride_x, int64_t row_stride_y) {
  if (!m || slot < 0 || slot > 1 || !x || !y || n < 1 || n > INT32_MAX) {
    set_error("dv_data_stream_open: bad arguments (n must be in [1, 2^31))");
    return DV_E_INVALID;
  }
  const Arch& A = m->A;
  const int64_t ex = (int64_t)A.H * A.H * A.C * (x_f64 ? 8 : 4), ey = (int64_t)A.H * A.H * A.C * (y_f64 ? 8 : 4);
  if ((n > 1 && (row_stride_x < ex && row_stride_x > -ex)) || (n > 1 && (row_stride_y < ey && row_stride_y > -ey))) {
    set_error("dv_data_stream_open: row strides %lld / %lld overlap rows of %lld / %lld bytes", (long long)row_stride_x,
              (long long)row_stride_y, (long long)ex, (long long)ey);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(m->ctx->device));
  // Nothing queued may still read the slot's old rows, and nothing prefetched may belong to them.  A queued step's input
  // normalised ahead (bf16 in_pre) whose step never ran - its enqueue failed, or a caller abandoned it - would otherwise
  // refuse every later training step: once all streams have drained no step can consume it, so it is dropped here.
  DV_TRY(ring_sync_streams(m));
  m->bn_pre_valid = false;
  m->bf.in_pre = false;
  m->bnpre_go_pending = false;
  DataSlot& d = m->slots[slot];
  if (d.x) (void)hipFree(d.x);
  if (d.y) (void)hipFree(d.y);
  d = DataSlot();
  DV_TRY(ring_get(m));
  d.streamed = true;
  d.hx = static_cast<const char*>(x);
  d.hy = static_cast<const char*>(y);
  d.x64 = x_f64 != 0;
  d.y64 = y_f64 != 0;
  d.sx = row_stride_x;
  d.sy = row_stride_y;
  d.n = n;
  return DV_OK;
}

int dv_data_info(dv_model* m, int32_t slot, int32_t* mode, int64_t* n, int64_t* h2d_bytes) {
  if (!m || slot < 0 || slot > 1) return DV_E_INVALID;
  const DataSlot& d = m->slots[slot];
  if (mode) *mode = d.streamed ? 2 : (d.x ? 1 : 0);
  if (n) *n = d.n;
  if (h2d_bytes) *h2d_bytes = d.h2d_bytes;
  return DV_OK;
}

int dv_ctx_mem_info(dv_ctx* c, int64_t* free_bytes, int64_t* total_bytes) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  size_t fr = 0, tot = 0;
  DV_HIP(hipMemGetInfo(&fr, &tot));
  if (free_bytes) *free_bytes = (int64_t)fr;
  if (total_bytes) *total_bytes = (int64_t)tot;
  return DV_OK;
}

int dv_data_upload(dv_model* m, int32_t slot, const float* x, const float* y, int64_t n) {
  if (!m || slot < 0 || slot > 1 || !x || !y || n < 1) {
    set_error("dv_data_upload: bad arguments");
    return DV_E_INVALID;
  }
  const Arch& A = m->A;
  if ((double)n * A.H * A.H * A.C >= 2147483648.0 * 64) {
    set_error("dataset too large");
    return DV_E_INVALID;
  }
  DV_TRY(dv_data_free(m, slot));
  m->bn_pre_valid = false;     // prefetched batch sums refer to the old rows
  if (m->bf.in_pre) {
    set_error("data uploaded while the input of a queued training step was prefetched");
    return DV_E_STATE;
  }
  size_t bytes = (size_t)n * A.H * A.H * A.C * sizeof(float);
  DataSlot& d = m->slots[slot];
  hipError_t e = hipMalloc((void**)&d.x, bytes);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(data x)", __FILE__, __LINE__);
  e = hipMalloc((void**)&d.y, bytes);
  if (e != hipSuccess) {
    (void)hipFree(d.x);
    d.x = nullptr;
    return hip_fail(e, "hipMalloc(data y)", __FILE__, __LINE__);
  }
  d.n = n;
  DV_HIP(hipMemcpy(d.x, x, bytes, hipMemcpyHostToDevice));
  DV_HIP(hipMemcpy(d.y, y, bytes, hipMemcpyHostToDevice));
  d.h2d_bytes = 2 * (int64_t)bytes;
  return DV_OK;
}

int dv_train_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t Bg,
                  const float* eps, uint64_t seed, float* out) {
  return run_step(m, MODE_TRAIN, slot, idx, first, B, Bg, eps, seed, out);
}
// Deferred results: the step is queued and its loss sums are copied to a pinned ring slot behind it; the host
// collects them later (dv_step_result), so a fit() loop can queue step k+1 before it looks at step k and the GPU
// does not idle while the host prepares the next batch (reference loop: train.py:27-37 Model.fit).
int dv_train_step_async(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t Bg,
                        uint64_t seed, int32_t ticket) {
  DV_TRY(check_step_args(m, slot, idx, first, B));
  if (ticket < 0 || ticket > 3) {
    set_error("ticket %d outside [0, 3]", ticket);
    return DV_E_INVALID;
  }
  if (m->ring_used[ticket]) {
    set_error("ticket %d has an uncollected result", ticket);
    return DV_E_STATE;
  }
  if (Bg <= 0) Bg = B;
  DV_HIP(hipSetDevice(m->ctx->device));
  if (!m->ring_scal) {
    DV_HIP(hipHostMalloc((void**)&m->ring_scal, 16 * sizeof(float), hipHostMallocDefault));
    DV_HIP(hipHostMalloc((void**)&m->ring_idx, (size_t)4 * m->Bc * sizeof(int), hipHostMallocDefault));
    for (auto& e : m->ring_ev) DV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // the caller's index array may be gone before the copy runs: the step's index vector is staged in pinned memory
  DV_TRY(enqueue_slot_step(m, MODE_TRAIN, slot, idx, first, B, Bg, nullptr, seed, m->ring_idx + (size_t)ticket * m->Bc));
  DV_HIP(hipMemcpyAsync(m->ring_scal + 4 * ticket, m->scal, 4 * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
  DV_HIP(hipEventRecord(m->ring_ev[ticket], m->ctx->stream));
  m->ring_bg[ticket] = Bg;
  m->ring_used[ticket] = true;
  return prof_flush(m);
}

int dv_step_result(dv_model* m, int32_t ticket, float* out) {
  if (!m || ticket < 0 || ticket > 3 || !m->ring_used[ticket]) {
    set_error("no queued step under ticket %d", ticket);
    return DV_E_STATE;
  }
  DV_HIP(hipEventSynchronize(m->ring_ev[ticket]));
  scalars_from_sums(m, m->ring_scal + 4 * ticket, m->ring_bg[ticket], out);
  m->ring_used[ticket] = false;
  return DV_OK;
}

int dv_eval_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t Bg, const float* eps,
                 uint64_t seed, float* out) {
  return run_step(m, MODE_EVAL, slot, idx, first, B, Bg, eps, seed, out);
}
int dv_grad_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t Bg, const float* eps,
                 uint64_t seed, float* out) {
  return run_step(m, MODE_GRAD, slot, idx, first, B, Bg, eps, seed, out);
}

int dv_train_steps(dv_model* m, int32_t slot, int64_t first, int32_t B, int32_t Bg, int32_t steps, uint64_t seed,
                   float* out) {
  if (steps < 1) return DV_E_INVALID;
  DV_TRY(check_step_args(m, slot, nullptr, 0, B));
  if (m->slots[slot].streamed) {
    set_error("dv_train_steps runs on resident data only (slot %d streams from host memory): use dv_train_step_async", slot);
    return DV_E_INVALID;
  }
  if (Bg <= 0) Bg = B;
  DV_HIP(hipSetDevice(m->ctx->device));
  int64_t span = std::max<int64_t>(1, m->slots[slot].n - B + 1);
  // DV_TIME_ENQUEUE=1: host time spent queuing the steps (stderr) - when it approaches the steps' GPU time the host, not the
  // GPU, paces the loop
  static const bool time_enqueue = DV_EXP_SWITCH("DV_TIME_ENQUEUE") != 0;   // (development library only)
  const auto tq0 = std::chrono::steady_clock::now();
  for (int k = 0; k < steps; ++k) {
    int64_t start = (first + (int64_t)k * B) % span;
    m->hint_next_first = k + 1 < steps ? (first + (int64_t)(k + 1) * B) % span : -1;   // lets step k prefetch k+1's BN sums
    DV_TRY(enqueue_step(m, MODE_TRAIN, m->slots[slot], nullptr, start, B, Bg, nullptr, seed + (uint64_t)k));
    if (m->prof_on) DV_TRY(prof_flush(m));
  }
  if (time_enqueue) {
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tq0).count();
    fprintf(stderr, "[dv] queued %d steps in %.1f us of host time (%.1f us per step)\n", steps, us, us / steps);
  }
  DV_TRY(fetch_scalars(m, Bg, out));
  return prof_flush(m);
}

static int infer_entry(dv_model* m, const void* x, bool x_f64, int64_t N, const float* eps, uint64_t seed, float* loc,
                       float* scale, float* mu, float* zstd, float* z) {
  if (!m || !x || N < 0) return DV_E_INVALID;
  const Arch& A = m->A;
  TinyCall tiny(m, N);
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  if (N > 256 && !m->prof_on) {
    PipeJob j;
    j.x = x;
    j.x_f64 = x_f64;
    j.N = N;
    j.chunk = infer_chunk(m, N);
    j.eps = eps;
    j.seed = seed;
    j.loc = loc;
    j.scale = scale;
    j.mu = mu;
    j.zstd = zstd;
    j.z = z;
    DV_TRY(infer_pipelined(m, j));
    return prof_flush(m);
  }
  std::vector<float> cast;
  for (int64_t o = 0; o < N; o += m->Bc) {
    int nb = (int)std::min<int64_t>(m->Bc, N - o);
    const float* xs;
    if (x_f64) {
      cast.resize((size_t)nb * stamp);
      const double* xd = static_cast<const double*>(x) + o * stamp;
      for (size_t i = 0; i < (size_t)nb * stamp; ++i) cast[i] = (float)xd[i];
      xs = cast.data();
    } else {
      xs = static_cast<const float*>(x) + o * stamp;
    }
    DV_TRY(stage_host_batch(m, xs, nb));
    auto run_forward = [&]() -> int {
      if (m->normalise) DV_TRY(launch_normalise(m->stage_x, (long)nb * stamp, false, s));
      DV_TRY(forward_all(m, m->stage_x, nullptr, nullptr, 0, nb, nb, false, false, false, eps ? eps + o * A.d : nullptr,
                         seed, (unsigned)m->ctx->rank, (unsigned)o, zstd != nullptr, false, true));
      if (m->normalise && loc) DV_TRY(launch_normalise(m->loc, (long)nb * stamp, true, s));
      return OK;
    };
    // Launch-bound sizes (one forward lane, a single chunk, engine-drawn noise): replay a captured graph.  The first
    // call of a size runs eagerly (kernel attributes and other one-time host work must not fall into a capture), the
    // second is captured.
    // Opt-in (dv_config.infer_graph): measured on MI355X a replay takes exactly as long as the
    // eager launches (0.600 vs 0.603 ms for one stamp, 0.806 vs 0.803 ms for 32) - the chain of ~45 dependent
    // few-microsecond kernels is bound by the GPU's dispatch-to-dispatch latency, not by host submission.
    const bool graphable = m->infer_graph && nb < 64 && N <= m->Bc && !eps && m->seed_dev != nullptr;
    if (graphable && m->graph_epoch != m->param_epoch) {
      // a parameter changed since the graphs were captured: the derived weights (Winograd transforms, bf16 casts, padded
      // head) are re-made at the head of an EAGER forward pass, which a replay does not contain - drop the graphs; the
      // next call of a size runs eagerly (and refreshes), the one after it is captured again
      for (auto& kv : m->infer_graphs) (void)hipGraphExecDestroy(kv.second);
      m->infer_graphs.clear();
      m->infer_seen.clear();
      m->graph_epoch = m->param_epoch;
    }
    if (graphable) {
      const int key = nb | (zstd ? 1 << 20 : 0) | (m->normalise ? 1 << 21 : 0) | (loc ? 1 << 22 : 0);
      m->use_seed_dev = true;
      const unsigned long long seed_host = seed;
      int st = OK;
      if (hipMemcpyAsync(m->seed_dev, &seed_host, sizeof seed_host, hipMemcpyHostToDevice, s) != hipSuccess) st = E_HIP;
      auto it = m->infer_graphs.find(key);
      if (st == OK && it != m->infer_graphs.end()) {
        if (hipGraphLaunch(it->second, s) != hipSuccess) st = E_HIP;
      } else if (st == OK && m->infer_seen[key]++ >= 1) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) st = E_HIP;
        if (st == OK) {
          st = run_forward();
          const hipError_t ce = hipStreamEndCapture(s, &g);       // always end the capture, also after an error
          if (st == OK && ce != hipSuccess) st = E_HIP;
        }
        if (st == OK && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) st = E_HIP;
        if (g) (void)hipGraphDestroy(g);
        if (st == OK) {
          m->infer_graphs[key] = ge;
          if (hipGraphLaunch(ge, s) != hipSuccess) st = E_HIP;
        }
      } else if (st == OK) {
        st = run_forward();
      }
      m->use_seed_dev = false;
      if (st != OK) {
        if (st == E_HIP) set_error("graph-captured inference forward failed: %s", hipGetErrorString(hipGetLastError()));
        return st;
      }
    } else {
      DV_TRY(run_forward());
    }
    if (loc) DV_HIP(hipMemcpyAsync(loc + o * stamp, m->loc, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    if (scale)
      DV_HIP(hipMemcpyAsync(scale + o * stamp, m->scale, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    if (mu)
      DV_HIP(hipMemcpy2DAsync(mu + o * A.d, A.d * sizeof(float), m->t, A.twp * sizeof(float), A.d * sizeof(float), nb,
                              hipMemcpyDeviceToHost, s));
    if (zstd) DV_TRY(copy_rows(zstd + o * A.d, A.d, m->zstd, A.dp, A.d, nb, hipMemcpyDeviceToHost, s));
    if (z) DV_TRY(copy_rows(z + o * A.d, A.d, m->z, A.dp, A.d, nb, hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
    m->lastB = nb;
  }
  return prof_flush(m);
}

int dv_model_set_keep_outputs(dv_model* m, int32_t on) {
  if (!m) return DV_E_INVALID;
  m->keep_outputs = on != 0;
  return DV_OK;
}


int dv_model_set_mse_sample(dv_model* m, int32_t on) {
  if (!m) return DV_E_INVALID;
  m->mse_sample = on != 0;
  return DV_OK;
}

int dv_model_set_normalise(dv_model* m, int32_t on) {
  if (!m) return DV_E_INVALID;
  m->normalise = on != 0;
  return DV_OK;
}

int dv_infer(dv_model* m, const float* x, int64_t N, const float* eps, uint64_t seed, float* loc, float* scale,
             float* mu, float* zstd, float* z) {
  return infer_entry(m, x, false, N, eps, seed, loc, scale, mu, zstd, z);
}

int dv_infer_f64(dv_model* m, const double* x, int64_t N, const float* eps, uint64_t seed, float* loc, float* scale,
                 float* mu, float* zstd, float* z) {
  return infer_entry(m, x, true, N, eps, seed, loc, scale, mu, zstd, z);
}

// ---- many fields in one call (dv_infer_fields, _keep, _composite) ------------------------------------------
// The stamps of M fields form one global list (field_ptr[m] .. field_ptr[m + 1] are cut from field m) that runs through the
// pipeline in the chunks dv_infer makes for N stamps, whatever field a stamp belongs to; stamp i draws Philox row i.  The
// fields are uploaded in groups of consecutive fields sized against free device memory; a group covers whole chunks, so a
// field whose stamps straddle two groups is resident in both (and its partly composited results travel with it).
// The single-field calls (dv_infer_cutouts*) are this with M = 1.
struct FieldsOut {                  // result fields of dv_infer_fields_composite, host [M][F][F][nb]; null otherwise
  double *mean = nullptr, *stddev = nullptr, *residual = nullptr, *mse = nullptr;
  double *epistemic = nullptr, *eps_norm = nullptr;   // dv_infer_fields_mc_composite: [M][F][F][nb] and [N]
  // dv_infer_fields_fit_composite: dist instead of the request's places, the fit's parameters and per-galaxy results (host [N])
  const double* dist = nullptr;
  double bound = 0.0;
  int max_iter = 0;
  double *shifts = nullptr, *objective = nullptr;
  int32_t *iters = nullptr, *status = nullptr;
};

struct MeasureOut {                 // the catalogue of dv_infer_fields_measure, host, rows = global stamp numbers
  dv_measure_params par{};
  double *flux = nullptr, *flux_err = nullptr, *shape = nullptr;   // [N][nb], [N][nb], [N][5]
  int32_t *iters = nullptr, *status = nullptr;                     // [N]
  double* mse = nullptr;            // [N], optional: mse_center of the catalogue-only call (no FieldsOut to carry it)
};

struct MeasureMcOut {               // the Monte-Carlo catalogue of dv_infer_fields_measure_mc, host, rows = global stamp numbers
  McState st{};                     // the per-sample rows given together or not at all
  int nsamples = 0;
  uint64_t seed = 0;                // of the decodes (the pass itself draws from the job's seed)
};

// the refusals every field-sourced call takes before any GPU work, and the two tables it works from: sfield[i] = the field
// of stamp i, fptr32 = field_ptr as the kernels read it.  places: the placements of a compositing call, or null.
static int fields_tables(dv_model* m, const char* who, int32_t M, const int64_t* field_ptr, int64_t N, int F, int nb,
                         const int32_t* starts, const int32_t* places, std::vector<int32_t>& sfield,
                         std::vector<int>& fptr32) {
  if (!m || !field_ptr || M < 0 || N < 0 || F < 1 || (N > 0 && !starts)) return DV_E_INVALID;
  const Arch& A = m->A;
  const int cs = A.H;
  if (nb != A.C || cs > F) {
    set_error("%s: the fields have %d bands and %d pixels, the network takes %d x %d x %d stamps", who, nb, F, cs, cs, A.C);
    return DV_E_INVALID;
  }
  // (the placements are checked below, each after its stamp's cutout: the order in which a call with both wrong is refused)
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, nullptr, nullptr, &sfield, &fptr32));
  for (int64_t i = 0; i < N; ++i) {
    const int x = starts[2 * i], y = starts[2 * i + 1];
    if (x < 0 || y < 0 || x > F - cs || y > F - cs) {   // (cs <= F holds; no x + cs: it overflows near INT_MAX)
      set_error("%s: cutout %ld of field %d (start %d,%d size %d) leaves the %d-pixel field", who, (long)i, sfield[i], x, y, cs, F);
      return DV_E_INVALID;
    }
    if (places) DV_TRY(place_check(who, i, places));
  }
  return DV_OK;
}

// ---- the many-field call, stage by stage ------------------------------------------------------------------------------------
// Every optional stage of the call owns its device buffers in one struct with three steps: allocate from the call's sizes,
// bind into the job (one nested PipeJob member), download into the caller's arrays.  What a stage adds to the memory a
// resident field costs stands beside its allocations (bytes_per_field / bytes_fixed); what it adds per stamp is the bytes()
// of the columns it states (rows.h).
struct FieldsCall {                 // the sizes of one call
  int64_t N, K;                     // stamps, chunks
  int F, nb, cs, chunk;
  hipStream_t s;
};

// device memory a call may fill with fields: 8/10 of what is free, less what the call allocates beside them, and at most
// DV_FIELDS_GROUP_MB
static int fields_budget(size_t reserve, size_t* budget) {
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  *budget = free_b / 10 * 8;
  *budget = *budget > reserve ? *budget - reserve : 0;
  if (const char* e = getenv("DV_FIELDS_GROUP_MB")) {
    const long mb = atol(e);
    if (mb > 0) *budget = std::min(*budget, (size_t)mb << 20);
  }
  return DV_OK;
}

// groups of consecutive fields, at most G resident at a time, each covering whole chunks: a field whose stamps straddle two
// groups is resident in both
struct FieldGroup { int64_t k0, k1; int f0, f1; };      // chunks [k0, k1), fields [f0, f1]
static int plan_field_groups(const char* who, const int32_t* sfield, int64_t N, int chunk, int64_t G,
                             std::vector<FieldGroup>& groups, int64_t* gmax) {
  const int64_t K = (N + chunk - 1) / chunk;
  *gmax = 0;
  for (int64_t k = 0; k < K;) {
    const int f0 = sfield[k * chunk];
    int64_t k1 = k;
    int f1 = f0;
    while (k1 < K) {
      const int last = sfield[std::min<int64_t>(N, (k1 + 1) * chunk) - 1];
      if ((int64_t)last - f0 + 1 > G) break;
      f1 = last;
      ++k1;
    }
    if (k1 == k) {
      set_error("%s: the %d stamps of chunk %ld come from %d fields, device memory holds %ld at a time: lower max_batch",
                who, chunk, (long)k, sfield[std::min<int64_t>(N, (k + 1) * chunk) - 1] - f0 + 1, (long)G);
      return DV_E_NOMEM;
    }
    groups.push_back({k, k1, f0, f1});
    *gmax = std::max<int64_t>(*gmax, f1 - f0 + 1);
    k = k1;
  }
  return DV_OK;
}

// a field without stamps: nothing predicted, nothing subtracted
static void fields_write_empty(const FieldsOut& fo, const double* fields, int32_t M, const int64_t* field_ptr, size_t felems) {
  const size_t fb = felems * sizeof(double);
  for (int32_t f = 0; f < M; ++f)
    if (field_ptr[f + 1] == field_ptr[f]) {
      memset(fo.mean + (size_t)f * felems, 0, fb);
      memset(fo.stddev + (size_t)f * felems, 0, fb);
      if (fo.epistemic) memset(fo.epistemic + (size_t)f * felems, 0, fb);
      if (fo.residual) memcpy(fo.residual + (size_t)f * felems, fields + (size_t)f * felems, fb);
    }
}

// one result stack of the resident group and the caller's [M][F][F][nb] array it ends up in (null: not wanted)
struct ResultStack {
  DevBuf<double> dev;
  double* host = nullptr;
  int alloc(double* h, size_t elems) { host = h; return h ? dev.alloc(elems) : DV_OK; }
  // a group begins: zeros, or the source fields for a residual
  int begin(const double* source, size_t bytes, hipStream_t s) {
    if (!host) return DV_OK;
    if (source) DV_HIP(hipMemcpyAsync(dev, source, bytes, hipMemcpyDeviceToDevice, s));
    else DV_HIP(hipMemsetAsync(dev, 0, bytes, s));
    return DV_OK;
  }
  // the group's first field was composited in part with the previous group: go on from those sums
  int carry(size_t goff, size_t fb, hipStream_t s) {
    if (host) DV_HIP(hipMemcpyAsync(dev, host + goff, fb, hipMemcpyHostToDevice, s));
    return DV_OK;
  }
  int end(size_t bytes, size_t goff, hipStream_t s) {
    if (host) DV_HIP(hipMemcpyAsync(host + goff, dev, bytes, hipMemcpyDeviceToHost, s));
    return DV_OK;
  }
};

struct CompositeStage {             // the mean / stddev / residual sums
  ResultStack mean, stddev, residual;
  static size_t bytes_per_field(const FieldsOut& fo, size_t fb) { return fb * (fo.residual ? 3 : 2); }
  int alloc(const FieldsOut& fo, size_t elems) {
    DV_TRY(mean.alloc(fo.mean, elems));
    DV_TRY(stddev.alloc(fo.stddev, elems));
    return residual.alloc(fo.residual, elems);
  }
  void bind(PipeJob::Sinks& k) const { k.mean_f = mean.dev; k.std_f = stddev.dev; k.res_f = residual.dev; }
};

struct MonteCarloStage {            // what the Monte-Carlo estimate adds: one more result field, one more scalar per stamp (7g)
  ResultStack eps;
  DevBuf<double> norm;
  double* norm_h = nullptr;
  static size_t bytes_per_field(const FieldsOut& fo, size_t fb) { return fo.epistemic ? fb : 0; }
  static size_t bytes_per_stamp(const FieldsOut& fo) { return fo.eps_norm ? sizeof(double) : 0; }
  int alloc(const FieldsOut& fo, size_t elems, int64_t N) {
    DV_TRY(eps.alloc(fo.epistemic, elems));
    norm_h = fo.eps_norm;
    return norm_h ? norm.alloc((size_t)N) : DV_OK;
  }
  void bind(PipeJob::Sinks& k) const { k.eps_f = eps.dev; k.eps_norm = norm; }
  int download(int64_t N, hipStream_t s) {
    if (!norm_h) return DV_OK;
    DV_HIP(hipMemcpyAsync(norm_h, norm, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
    return DV_OK;
  }
};

struct FitStage {                   // the position fit and the fractional placements (7i)
  PosfitPlanOwner plan;             // (the plan's device copy goes with it)
  std::vector<int> l0;
  size_t coef_doubles = 0;
  DevBuf<double> img, totsq, dist, stamps, work, shifts, obj, coef;
  DevBuf<int> iters, status;
  DevBuf<char> objs;
  // the plan: every galaxy's windows, laid out chunk by chunk against field 0 (rebased once the groups are known)
  int make_plan(const FieldsOut& fo, const FieldsCall& c, const int32_t* sfield) {
    PosfitPlan* p = nullptr;
    DV_TRY(posfit_plan_create(c.F, c.cs, (int)c.N, fo.dist, fo.shifts, fo.bound, fo.max_iter, &p));
    plan.reset(p);
    l0.resize((size_t)c.K + 1);
    for (int64_t k = 0; k < c.K; ++k)
      l0[k] = posfit_plan_layout(plan.get(), (int)(k * c.chunk), (int)std::min<int64_t>(c.N, (k + 1) * c.chunk), c.chunk, sfield, 0,
                                 (int)(k * c.chunk));
    l0[c.K] = posfit_plan_launch_count(plan.get());
    coef_doubles = scene_frac_coef_doubles(c.cs, c.nb, fo.epistemic ? 3 : 2);
    return DV_OK;
  }
  static size_t bytes_per_field(int F) { return ((size_t)F * F + 1) * sizeof(double); }   // an r-band plane and its sum of squares
  // allocated once per call: the fit's workspace, the coefficient workspace of the fractional compositing, a chunk's r-band
  // stamps and placements, the plan's device copy and the per-galaxy arrays
  size_t bytes_fixed(const FieldsCall& c) const {
    return ((size_t)posfit_plan_work_doubles(plan.get()) + coef_doubles + (size_t)c.chunk * c.cs * c.cs) * sizeof(double) +
           scene_frac_obj_bytes((size_t)c.chunk) + posfit_plan_geom_bytes((size_t)c.N) +
           (size_t)c.N * (5 * sizeof(double) + 2 * sizeof(int));
  }
  int alloc(const FieldsOut& fo, const FieldsCall& c, int64_t gmax, const std::vector<FieldGroup>& groups) {
    const size_t n = (size_t)c.N;
    DV_TRY(img.alloc((size_t)gmax * c.F * c.F));
    DV_TRY(totsq.alloc((size_t)gmax));
    for (DevBuf<double>* b : {&dist, &shifts}) DV_TRY(b->alloc(2 * n));
    DV_TRY(obj.alloc(n));
    for (DevBuf<int>* b : {&iters, &status}) DV_TRY(b->alloc(n));
    DV_TRY(stamps.alloc((size_t)c.chunk * c.cs * c.cs));
    DV_TRY(work.alloc((size_t)posfit_plan_work_doubles(plan.get())));
    DV_TRY(coef.alloc(coef_doubles));
    DV_TRY(objs.alloc(scene_frac_obj_bytes((size_t)c.chunk)));
    DV_HIP(hipMemcpyAsync(dist, fo.dist, 2 * n * sizeof(double), hipMemcpyHostToDevice, c.s));
    DV_HIP(hipMemcpyAsync(shifts, fo.shifts, 2 * n * sizeof(double), hipMemcpyHostToDevice, c.s));
    for (const FieldGroup& g : groups)
      posfit_plan_rebase(plan.get(), (int)(g.k0 * c.chunk), (int)std::min<int64_t>(c.N, g.k1 * c.chunk), g.f0);
    return posfit_plan_upload(plan.get(), c.s);
  }
  void bind(PipeJob::Fit& f) const {
    f.plan = plan.get(); f.l0 = l0.data();
    f.img = img; f.totsq = totsq; f.dist_d = dist;
    f.stamps = stamps; f.work = work;
    f.shifts_d = shifts; f.obj = obj; f.iters = iters; f.status = status;
    f.objs_d = objs.get(); f.coef_d = coef;
  }
  // a group begins: the r band of its resident fields as planes
  int begin(const double* fields_d, size_t ng, const FieldsCall& c) {
    DV_TRY(launch_posfit_band_f64(fields_d, (long)ng * c.F * c.F, c.nb, 2, img, c.s));
    return launch_posfit_total_sq(img, (int)ng, (long)c.F * c.F, totsq, c.s);
  }
  int download(const FieldsOut& fo, int64_t N, hipStream_t s) {
    DV_HIP(hipMemcpyAsync(fo.shifts, shifts, (size_t)N * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(fo.objective, obj, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(fo.iters, iters, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(fo.status, status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
    return DV_OK;
  }
};

// The stages that add per-stamp rows state their columns (columns(): no GPU work, so the call's reserve can count
// rows.bytes() before anything is allocated), allocate them with rows.alloc(N) and end with rows_download.
static int rows_download(const Rows& rows, int64_t N, hipStream_t s) {
  DV_TRY(rows.download(0, N, s));
  DV_HIP(hipStreamSynchronize(s));
  return DV_OK;
}

// The reserve of a many-field call has always counted one double per stamp more than the catalogue allocates.  It is slack, not
// a column; it stays because the DV_FIELDS_GROUP_MB tests pin group boundaries that were computed with it.
constexpr size_t CATALOGUE_RESERVE_SLACK = sizeof(double);

struct CatalogueStage {             // fluxes, errors and adaptive moments of every stamp (7j)
  CatRows dev{};
  Rows rows;
  void columns(const MeasureOut& mo, int nb) {
    catalogue_columns(rows, dev, CatRows{mo.flux, mo.flux_err, mo.shape, mo.iters, mo.status}, nb, true);
  }
  void bind(PipeJob::Measure& q, const dv_measure_params& par) const {
    q.flux = dev.flux; q.ferr = dev.flux_err; q.shape = dev.shape; q.iters = dev.iters; q.status = dev.status;
    q.band = par.band; q.max_iter = par.max_iter; q.sigma0 = par.sigma0; q.tol = par.tol;
  }
};

struct CatalogueMcStage {           // means and standard deviations over the Monte-Carlo decodes of every stamp (7k)
  McState dev{};                    // the results (and running state) of a stamp, with or without its per-sample rows
  McScratch w{};                    // the scratch rows of one decoder pass: at most the workspace capacity
  Rows rows, scratch;
  void columns(const MeasureMcOut& o, int nb, bool keep) {
    mc_columns(rows, dev, o.st, nb, o.nsamples, keep);
    mc_scratch_columns(scratch, w, nb, 1);
  }
  int alloc(int64_t N, int Bc) {
    DV_TRY(rows.alloc(N));
    return scratch.alloc(Bc);
  }
  void bind(PipeJob::MeasureMc& q, const dv_measure_params& par) const {
    q.st = dev;
    q.w = w;
    q.band = par.band; q.max_iter = par.max_iter; q.sigma0 = par.sigma0; q.tol = par.tol;
  }
};

struct BlendOut { double* blend = nullptr; int32_t* npix = nullptr; };   // dv_infer_fields_measure_blend, host [N][4], [N]

struct MeanFieldStage {             // the device-side mean field of a catalogue-only call (7l, 7p): what the stages that read the
  DevBuf<double> mean;              // completed composite get where no composite stage runs; empty with result fields
  static size_t bytes_per_field(bool own_mean, size_t fb) { return own_mean ? fb : 0; }
  int alloc(bool own_mean, size_t elems) { return own_mean ? mean.alloc(elems) : DV_OK; }
  void bind(PipeJob::MeanField& q) const { q.mean_f = mean; }
  // a group begins: zeros, but for a first field that was composited in part with the previous group, whose sums lie in slot
  // `from` and go on in slot 0
  int begin(size_t ng, size_t felems, long from, hipStream_t s) {
    if (!mean) return DV_OK;
    const size_t fb = felems * sizeof(double);
    if (from > 0) DV_HIP(hipMemcpyAsync(mean, mean.get() + (size_t)from * felems, fb, hipMemcpyDeviceToDevice, s));
    const size_t keep = from >= 0 ? 1 : 0;
    if (ng > keep) DV_HIP(hipMemsetAsync(mean.get() + keep * felems, 0, (ng - keep) * fb, s));
    return DV_OK;
  }
};

struct BlendStage {                 // the blendedness sums of every stamp (7l)
  BlendRows dev{};
  Rows rows;
  void columns(const BlendOut& o) { blend_columns(rows, dev, BlendRows{o.blend, o.npix}); }
  void bind(PipeJob::Blend& q) const { q.blend = dev.blend; q.npix = dev.npix; }
};

struct RegaussOut {                 // dv_infer_fields_measure_psf: the PSFs and the index in, the corrected rows out (host)
  const double* psf = nullptr;      // [K][ps][ps]
  int K = 0, ps = 0;
  const int32_t* index = nullptr;   // [N]
  double psf_sigma0 = 0.0;
  double* out = nullptr;            // [N][6]
  int32_t *iters = nullptr, *status = nullptr;           // [N]
  double *psf_shape = nullptr, *psf_aux = nullptr;       // [K][5], [K][3]
  int32_t *psf_iters = nullptr, *psf_status = nullptr;   // [K]
};

struct RegaussStage {               // the PSF-corrected moments of every stamp (7n)
  RegaussPsf psf;
  RegaussRows dev{};
  Rows rows;
  DevBuf<int> index;                // every stamp's PSF: an input, uploaded once
  void columns(const RegaussOut& o) { regauss_columns(rows, dev, RegaussRows{o.out, o.iters, o.status}); }
  size_t bytes_per_stamp() const { return rows.bytes() + sizeof(int); }
  static size_t bytes_fixed(const RegaussOut& o) { return RegaussPsf::bytes(o.K, o.ps); }
  // the per-stamp rows, and the PSFs uploaded and measured on the call's stream: once, before the first chunk
  int alloc(const RegaussOut& o, int64_t N, const dv_measure_params& par, hipStream_t s) {
    DV_TRY(psf.alloc(o.K, o.ps));
    DV_TRY(rows.alloc(N));
    DV_TRY(index.alloc((size_t)N));
    DV_HIP(hipMemcpyAsync(index, o.index, (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
    return psf.measure(o.psf, o.K, o.ps, o.psf_sigma0, par.tol, par.max_iter, s);
  }
  void bind(PipeJob::Regauss& q, const RegaussOut& o) const {
    q.psf = &psf; q.K = o.K; q.ps = o.ps; q.index = index; q.out = dev.out; q.iters = dev.iters; q.status = dev.status;
  }
  int download(const RegaussOut& o, int64_t N, hipStream_t s) {
    DV_TRY(rows.download(0, N, s));
    DV_TRY(psf.download(o.K, o.psf_shape, o.psf_aux, o.psf_iters, o.psf_status, s));
    DV_HIP(hipStreamSynchronize(s));
    return DV_OK;
  }
};

struct ApertureOut {                // dv_infer_fields_measure_aper: the parameters in, the photometry rows out (host)
  ApertureParams par{};
  ApertureRows rows{};
};

struct ApertureStage {              // the aperture photometry of every stamp (7o)
  ApertureRows dev{};
  Rows rows;
  void columns(const ApertureOut& o, int nb) { aperture_columns(rows, dev, o.rows, o.par, nb, true); }
  void bind(PipeJob::Aper& q, const ApertureOut& o) const { q.on = true; q.par = o.par; q.rows = dev; }
};

struct ApertureFieldOut { ApertureFieldRows rows{}; };   // dv_infer_fields_measure_aper_data: the six field rows out (host)

struct ApertureFieldStage {         // the apertures of every stamp on the mean field and the source field (7p)
  ApertureFieldRows dev{};
  Rows rows;
  void columns(const ApertureFieldOut& h, const ApertureOut& o, int nb) { aperture_field_columns(rows, dev, h.rows, o.par, nb); }
};

// dv_infer_fields_measure_fit: the parameters in, five rows out (host); _fit_weighted (7s): the host weight fields [M][F][F][nb]
// in too, and the rows carry fit_chi2 and fit_npix
// _fit_sky (7t): the order of the sky fitted jointly (-1: none) and its per-field outputs (host)
// _fit_nonneg (7u): the non-negativity constraint, max_iter and its per-field outputs (host)
// _fit_groups (7w): the fit by blend groups - group / group_size [N] (host), written at the seam by the host's grouping
// (FitFluxOut, common.h: the request every caller of the fit fills)

struct FitFluxStage {               // the simultaneous flux fit of every field's mean stamps to its source field (7q)
  DevBuf<float> store;              // the mean stamps of all N stamps: a field's are read when its composite is complete
  FitFluxWork work;
  FitGroupsWork gwork;              // the fit by blend groups (7w): its tables and scratch grow at the seam as the fields need
  FitFluxRows dev{};
  Rows rows;
  FitFluxFieldOut fields;           // the per-field outputs of a fit with sky (7t) or non-negative (7u), downloaded at the seam
  void columns(const FitFluxOut& o, int nb) { fitflux_columns(rows, dev, o.rows, nb, o.weights != nullptr, o.nonneg.on); }
  size_t bytes_per_stamp(int cs, int nb) const { return (size_t)cs * cs * nb * sizeof(float) + rows.bytes(); }
  int alloc(const FitFluxPlan& plan, int64_t N, int64_t M, int cs, int nb, bool weighted, const FitFluxNonneg& nn) {
    DV_TRY(store.alloc((size_t)N * cs * cs * nb));
    DV_TRY(work.alloc(plan, M, weighted));
    DV_TRY(fields.alloc(plan.q, nn, (size_t)M, nb));
    return rows.alloc(N);
  }
  void bind(PipeJob::FitFlux& q) const { q.store = store; }
};

// dv_infer_fields_measure_moments_data (7x): the optional host weight fields [M][F][F][nb] in, the five rows out (host)
struct MomentsFieldOut { MomentsFieldRows rows{}; const double* weights = nullptr; };

struct MomentsFieldStage {          // the adaptive moments of every galaxy's child image D - T + P (7x)
  DevBuf<float> store;              // the mean stamps of all N stamps, unless the flux fit keeps them already
  DevBuf<double> wdev;              // the resident group of weight fields, unless the flux fit has uploaded the same ones
  MomentsFieldRows dev{};
  Rows rows;
  void columns(const MomentsFieldOut& o, int nb) { moments_field_columns(rows, dev, o.rows, nb); }
  size_t bytes_per_stamp(int cs, int nb, bool own_store) const {
    return (own_store ? (size_t)cs * cs * nb * sizeof(float) : 0) + rows.bytes();
  }
  int alloc(int64_t N, int cs, int nb, bool own_store, size_t welems) {
    if (own_store) DV_TRY(store.alloc((size_t)N * cs * cs * nb));
    if (welems) DV_TRY(wdev.alloc(welems));
    return rows.alloc(N);
  }
  void bind(PipeJob::FitFlux& q) const { if (store) q.store = store; }
};

// What a many-field call wants back, beside what its PipeJob streams to the host: each part is there or not.
struct FieldsRequest {
  std::optional<FieldsOut> fields;              // the composited result fields
  std::optional<MeasureOut> cat;                // the catalogue
  // the extras hang off the catalogue - they read its parameters or its device rows - and are given only with `cat`
  std::optional<MeasureMcOut> mc;
  std::optional<BlendOut> blend;
  std::optional<RegaussOut> regauss;
  std::optional<ApertureOut> aper;
  std::optional<ApertureFieldOut> aper_field;   // reads the aperture rows: only with `aper`
  std::optional<FitFluxOut> fit_flux;
  std::optional<MomentsFieldOut> moments;       // reads the completed composite, the source field and the kept mean stamps
  // host [N][2], where every stamp lies in its field.  Read when the call composites - result fields without a position fit,
  // or a stage at the completed-field seam (blend, aper_field, fit_flux, moments), with or without result fields - and not otherwise
  const int32_t* places = nullptr;
};

// j: the host side of the job - fields, starts, seed, the host outputs, consumer and Monte-Carlo stage the caller wants;
// the device side and the rows are filled in here
static int infer_fields_impl(dv_model* m, const char* who, int32_t M, const int64_t* field_ptr, int64_t N, PipeJob j,
                             const FieldsRequest& rq) {
  // check
  if (((rq.mc || rq.blend || rq.regauss || rq.aper || rq.aper_field || rq.fit_flux || rq.moments) && !rq.cat) || (rq.aper_field && !rq.aper)) {
    set_error("%s: the extras of a catalogue go with the catalogue, the apertures on the fields with the aperture rows", who);
    return DV_E_INVALID;
  }
  const double* fields = j.fields;
  const int F = j.F, nb = j.nb;
  if (M > 0 && !fields) return DV_E_INVALID;
  std::vector<int32_t> sfield;
  std::vector<int> fptr32;
  const int32_t* places = rq.fields || rq.blend || rq.aper_field || rq.fit_flux || rq.moments ? rq.places : nullptr;
  DV_TRY(fields_tables(m, who, M, field_ptr, N, F, nb, j.starts, places, sfield, fptr32));
  const size_t felems = (size_t)F * F * nb, fb = felems * sizeof(double);
  FitFluxPlan ffplan;
  const bool ff_groups = rq.fit_flux && rq.fit_flux->grouped();   // (7w: no plan by field - the groups are known at the seam)
  if (rq.fit_flux && !ff_groups)                       // (before anything is written or queued)
    DV_TRY(fitflux_plan(who, field_ptr, M, nb, rq.fit_flux->par, &ffplan, rq.fit_flux->sky_order, F));
  if (rq.fit_flux && rq.fit_flux->nonneg.on && M > 0) {   // (7u: a field without unknowns has no factorisation and converged)
    std::fill(rq.fit_flux->nonneg.iters, rq.fit_flux->nonneg.iters + (size_t)M * nb, 0);
    std::fill(rq.fit_flux->nonneg.status, rq.fit_flux->nonneg.status + (size_t)M * nb, 0);
  }
  if (rq.fields) fields_write_empty(*rq.fields, fields, M, field_ptr, felems);
  // A fit with sky (7t) solves the fields without galaxies too.  The seam below reaches the fields of a group; every other one
  // - the call without stamps, the empty fields before the first group, between two groups and behind the last - takes the
  // host-array path, whose field sums have the same bits: they depend on the field alone.
  auto sky_alone = [&](int fa, int fz) -> int {        // the empty fields fa .. fz - 1
    if (fz <= fa) return DV_OK;
    FitFluxOut o = *rq.fit_flux;                       // the same request, its per-field outputs and weights from field fa on
    const size_t q = (size_t)ffplan.q, e = (size_t)fa * nb;
    const std::vector<int64_t> none((size_t)(fz - fa) + 1, 0);
    o.sky = FitFluxSky{-1, o.sky.coef + e * q, o.sky.cov + e * q * q, o.sky.status + e * q, o.sky.npix + e};
    if (o.nonneg.on) o.nonneg.iters += e, o.nonneg.status += e;
    if (o.weights) o.weights += (size_t)fa * felems;
    o.who = who;
    return scene_fit_flux(nullptr, nullptr, none.data(), 0, m->A.H, nb, fields + (size_t)fa * felems, fz - fa, F, o, m->ctx->device,
                          m->ctx->stream);
  };
  const bool ff_sky = rq.fit_flux && ffplan.q != 0;
  if (N == 0) return ff_sky ? sky_alone(0, M) : DV_OK;
  TinyCall tiny(m, N);
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const int chunk = infer_chunk(m, N);
  const FieldsCall c{N, (N + chunk - 1) / chunk, F, nb, m->A.H, chunk, s};
  InferPipe* pipe = nullptr;
  DV_TRY(pipe_get(m, chunk, &pipe, !rq.fields && !rq.cat));   // before the budget below: the pipeline's buffers come first
  // plan the groups: fields per group = what free memory holds beside the per-stamp tables and the stages' own arrays
  const bool fitting = rq.fields && rq.fields->dist;
  double* mse_h = rq.fields ? rq.fields->mse : rq.cat ? rq.cat->mse : nullptr;
  DevBuf<double> fdev;                                // the resident group of source fields
  DevBuf<double> wdev;                                // ... and of their weight fields, in a weighted flux fit (7s)
  const double* wfields = rq.fit_flux ? rq.fit_flux->weights : nullptr;
  StampTables tab;
  CompositeStage comp; MonteCarloStage mc; FitStage fit; CatalogueStage cat; CatalogueMcStage catmc; BlendStage bls; RegaussStage rgs; ApertureStage aps; MeanFieldStage mfs; ApertureFieldStage afs; FitFluxStage ffs; MomentsFieldStage mds;   // (a stage that does not run stays empty)
  ResultStack* const stacks[] = {&comp.mean, &comp.stddev, &mc.eps, &comp.residual};   // in the order their copies are queued
  if (fitting) DV_TRY(fit.make_plan(*rq.fields, c, sfield.data()));
  size_t per_field = fb, reserve = StampTables::bytes((size_t)N, (size_t)M);
  if (rq.fields) {
    per_field += CompositeStage::bytes_per_field(*rq.fields, fb) + MonteCarloStage::bytes_per_field(*rq.fields, fb);
    reserve += (size_t)N * MonteCarloStage::bytes_per_stamp(*rq.fields);
  }
  if (fitting) {
    per_field += FitStage::bytes_per_field(F);
    reserve += fit.bytes_fixed(c);
  }
  // the row sets state their columns: what they add to the reserve is derived from those
  if (rq.cat) {
    cat.columns(*rq.cat, nb);
    reserve += (size_t)N * (cat.rows.bytes() + CATALOGUE_RESERVE_SLACK);
  }
  if (rq.mc) {
    catmc.columns(*rq.mc, nb, rq.mc->st.sample_flux != nullptr);
    reserve += (size_t)N * catmc.rows.bytes() + (size_t)m->Bc * catmc.scratch.bytes();
  }
  const bool own_mean = (rq.blend || rq.aper_field || rq.moments) && !rq.fields;   // a stage reads the completed composite and no composite stage runs
  per_field += MeanFieldStage::bytes_per_field(own_mean, fb);
  if (rq.blend) {
    bls.columns(*rq.blend);
    reserve += (size_t)N * bls.rows.bytes();
  }
  if (rq.regauss) {
    rgs.columns(*rq.regauss);
    reserve += (size_t)N * rgs.bytes_per_stamp() + RegaussStage::bytes_fixed(*rq.regauss);
  }
  if (rq.aper) {
    aps.columns(*rq.aper, nb);
    reserve += (size_t)N * aps.rows.bytes();
  }
  if (rq.aper_field) {
    afs.columns(*rq.aper_field, *rq.aper, nb);
    reserve += (size_t)N * afs.rows.bytes();
  }
  if (rq.fit_flux) {
    ffs.columns(*rq.fit_flux, nb);
    reserve += (size_t)N * ffs.bytes_per_stamp(c.cs, nb) + FitFluxWork::bytes(ffplan, (size_t)M, wfields != nullptr) +
               FitFluxFieldOut::bytes(ffplan.q, rq.fit_flux->nonneg.on, (size_t)M, nb);
    // (a fit without sky has always set a counting-pixel row per field and band aside that nothing allocates: the group
    // boundaries follow from the reserve to the byte, so it stays)
    if (!ffplan.q) reserve += (size_t)M * nb * sizeof(long long);
    if (wfields) per_field += fb;
    if (ff_groups) {                                   // the tables of the grouping per stamp, and the scratch: at most the
      int64_t nmax = 0;                                // dense matrices of the largest field, at most scratch_bytes
      for (int f = 0; f < M; ++f) nmax = std::max(nmax, field_ptr[f + 1] - field_ptr[f]);
      reserve += (size_t)N * FitGroupsWork::BYTES_PER_ROW +
                 std::min((size_t)rq.fit_flux->par.scratch_bytes, (size_t)nb * (size_t)nmax * (size_t)nmax * sizeof(double));
    }
  }
  // (7x) the moments keep the mean stamps and upload the weight fields themselves unless the flux fit does either already
  const double* mwfields = rq.moments ? rq.moments->weights : nullptr;
  const bool md_store = rq.moments && !rq.fit_flux, md_wdev = mwfields && mwfields != wfields;
  if (rq.moments) {
    mds.columns(*rq.moments, nb);
    reserve += (size_t)N * mds.bytes_per_stamp(c.cs, nb, md_store);
    if (md_wdev) per_field += fb;
  }
  size_t budget = 0;
  DV_TRY(fields_budget(reserve, &budget));
  const int64_t G = (int64_t)(budget / per_field);
  if (G < 1) {
    set_error("%s: one %d-pixel field needs %zu bytes of device memory (field%s%s), %zu are available for fields", who, F,
              per_field, rq.fields ? " and its result fields" : own_mean ? " and its device-side mean field" : "",
              wfields || mwfields ? " and its weight field" : "", budget);
    return DV_E_NOMEM;
  }
  std::vector<FieldGroup> groups;
  int64_t gmax = 0;
  DV_TRY(plan_field_groups(who, sfield.data(), N, chunk, G, groups, &gmax));
  // allocate the stages and bind them into the job; from here on a failure waits for the streams before the buffers go
  StreamDrain drain(s, pipe->s_in, pipe->s_out);
  const size_t gelems = (size_t)gmax * felems;
  DV_TRY(fdev.alloc(gelems));
  if (wfields) DV_TRY(wdev.alloc(gelems));
  if (rq.fields) {
    DV_TRY(comp.alloc(*rq.fields, gelems));
    DV_TRY(mc.alloc(*rq.fields, gelems, N));
    comp.bind(j.sinks);
    mc.bind(j.sinks);
  }
  if (rq.cat) {
    DV_TRY(cat.rows.alloc(N));
    cat.bind(j.ms, rq.cat->par);
  }
  if (rq.mc) {
    DV_TRY(catmc.alloc(N, m->Bc));
    catmc.bind(j.mcm, rq.cat->par);
  }
  DV_TRY(mfs.alloc(own_mean, gelems));
  mfs.bind(j.mf);
  if (rq.blend) {
    DV_TRY(bls.rows.alloc(N));
    bls.bind(j.bl);
  }
  if (rq.regauss) {
    DV_TRY(rgs.alloc(*rq.regauss, N, rq.cat->par, s));
    rgs.bind(j.rg, *rq.regauss);
  }
  if (rq.aper) {
    DV_TRY(aps.rows.alloc(N));
    aps.bind(j.ap, *rq.aper);
  }
  if (rq.aper_field) DV_TRY(afs.rows.alloc(N));
  if (rq.fit_flux) {
    DV_TRY(ffs.alloc(ffplan, N, M, c.cs, nb, wfields != nullptr, rq.fit_flux->nonneg));
    ffs.bind(j.ff);
  }
  if (rq.moments) {
    DV_TRY(mds.alloc(N, c.cs, nb, md_store, md_wdev ? gelems : 0));
    mds.bind(j.ff);
  }
  if (fitting) {
    DV_TRY(fit.alloc(*rq.fields, c, gmax, groups));
    fit.bind(j.fit);
  }
  DV_TRY(tab.upload(N, M, j.starts, !fitting ? places : nullptr, sfield.data(), fptr32.data(), mse_h != nullptr, 0, s));
  j.fields_d = fdev;
  j.starts_d = tab.starts;
  j.sfield = sfield.data();
  j.sfield_d = tab.sfield;
  j.fptr_d = tab.fptr;
  j.chunk = chunk;
  j.sinks.places_d = tab.places;
  j.sinks.mse = tab.mse;
  // per group: upload -> the pipeline -> download the sinks
  int prev_last = -1, prev_first = -1;
  int sky_next = 0;                                    // with sky: the first field that has not been fitted yet
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const FieldGroup& g = groups[gi];
    const size_t ng = (size_t)(g.f1 - g.f0 + 1), goff = (size_t)g.f0 * felems;
    DV_HIP(hipMemcpyAsync(fdev, fields + goff, ng * fb, hipMemcpyHostToDevice, s));
    if (wfields) DV_HIP(hipMemcpyAsync(wdev, wfields + goff, ng * fb, hipMemcpyHostToDevice, s));
    if (md_wdev) DV_HIP(hipMemcpyAsync(mds.wdev, mwfields + goff, ng * fb, hipMemcpyHostToDevice, s));
    for (ResultStack* r : stacks) DV_TRY(r->begin(r == &comp.residual ? fdev.get() : nullptr, ng * fb, s));
    if (g.f0 == prev_last)
      for (ResultStack* r : stacks) DV_TRY(r->carry(goff, fb, s));
    if (fitting) DV_TRY(fit.begin(fdev, ng, c));
    DV_TRY(mfs.begin(ng, felems, g.f0 == prev_last ? (long)(prev_last - prev_first) : -1, s));
    DV_HIP(hipStreamSynchronize(s));               // the gather runs on the pipeline's copy stream
    j.f0 = g.f0;
    j.row0 = g.k0 * chunk;
    j.N = std::min<int64_t>(N, g.k1 * chunk) - j.row0;
    DV_TRY(infer_pipelined(m, j));
    if (rq.blend || rq.aper_field || rq.fit_flux || rq.moments) {
      // the completed-field seam: every field of the group has all its stamps composited now, but for a last field that
      // the next group goes on with (it is complete there); the parent sums and the field apertures of the complete fields'
      // galaxies - one contiguous range of rows - read the mean field, the source field and the rows where they lie
      const int fa = g.f0, fz = gi + 1 < groups.size() && groups[gi + 1].f0 == g.f1 ? g.f1 - 1 : g.f1;
      if (fz >= fa) {
        const int r0 = fptr32[fa], r1 = fptr32[fz + 1];
        const double* mean_f = rq.fields ? comp.mean.dev.get() : mfs.mean.get();
        if (rq.blend)
          DV_TRY(launch_blend_parent(cat.dev.shape + (size_t)r0 * 5, cat.dev.status + r0, tab.places.get() + 2 * (size_t)r0,
                                     tab.sfield.get() + r0, g.f0, r1 - r0, c.cs, nb, rq.cat->par.band, F, mean_f, fdev,
                                     bls.dev.blend + (size_t)r0 * 4, s));
        if (rq.aper_field)
          DV_TRY(launch_aperture_field(cat.dev.shape + (size_t)r0 * 5, cat.dev.status + r0,
                                       aps.dev.kron + (size_t)r0 * 3, aps.dev.status + r0,
                                       tab.places.get() + 2 * (size_t)r0, tab.sfield.get() + r0, g.f0, r1 - r0, c.cs, nb, F,
                                       mean_f, fdev, rq.aper->par, aperture_field_rows_at(afs.dev, r0, rq.aper->par, nb), s));
        // the stamps of the group's fields as the fit and the moments read them: the stamp store, the placements and the tables
        // count from stamp 0 of the call, the resident fields from g.f0
        FieldStamps fv{md_store ? mds.store.get() : ffs.store.get(), tab.places, tab.sfield, tab.fptr, fdev,
                       wfields ? wdev.get() : nullptr, mean_f, g.f0, c.cs, nb, F};
        if (ff_groups)                 // (7w: the groups' rows go to the host arrays here; the call's fields are the tables')
          DV_TRY(launch_fit_flux_groups(who, fv, fptr32.data(), fa, fz, 0, rq.fit_flux->par, ffs.gwork, ffs.dev,
                                        rq.fit_flux->group, rq.fit_flux->group_size, nullptr, s));
        else if (rq.fit_flux)
          DV_TRY(launch_fit_flux(fv, places, fptr32.data(), fa, fz, rq.fit_flux->par, ffs.work, ffs.dev, ffs.fields.sky,
                                 ffs.fields.nonneg, true, s));
        if (rq.moments) {              // (7x: its own mask, whatever the fit weighs with)
          fv.weight = md_wdev ? mds.wdev.get() : mwfields ? wdev.get() : nullptr;
          DV_TRY(launch_moments_field(fv, fptr32.data(), fa, fz, rq.cat->par.band, rq.cat->par.sigma0, rq.cat->par.tol,
                                      rq.cat->par.max_iter, mds.dev, s));
        }
        if (rq.fit_flux && (ff_sky || rq.fit_flux->nonneg.on)) {
          DV_TRY(ffs.fields.download(rq.fit_flux->sky, rq.fit_flux->nonneg, (size_t)fa, (size_t)fa, (size_t)(fz - fa + 1), nb, s));
          DV_HIP(hipStreamSynchronize(s));
        }
        if (ff_sky) {
          DV_TRY(sky_alone(sky_next, fa));
          sky_next = fz + 1;
        }
      }
    }
    if (rq.fields) {
      for (ResultStack* r : stacks) DV_TRY(r->end(ng * fb, goff, s));
      DV_HIP(hipStreamSynchronize(s));
    }
    prev_last = g.f1;
    prev_first = g.f0;
  }
  // download the per-stamp results
  if (mse_h) {
    DV_HIP(hipMemcpyAsync(mse_h, tab.mse, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
  }
  if (rq.cat) DV_TRY(rows_download(cat.rows, N, s));
  if (rq.mc) DV_TRY(rows_download(catmc.rows, N, s));
  if (rq.blend) DV_TRY(rows_download(bls.rows, N, s));
  if (rq.regauss) DV_TRY(rgs.download(*rq.regauss, N, s));
  if (rq.aper) DV_TRY(rows_download(aps.rows, N, s));
  if (rq.aper_field) DV_TRY(rows_download(afs.rows, N, s));
  if (rq.fit_flux) DV_TRY(rows_download(ffs.rows, N, s));
  if (rq.moments) DV_TRY(rows_download(mds.rows, N, s));
  if (ff_sky) DV_TRY(sky_alone(sky_next, M));
  if (rq.fields) DV_TRY(mc.download(N, s));
  if (fitting) DV_TRY(fit.download(*rq.fields, N, s));
  drain.dismiss();
  return prof_flush(m);
}

// the host side of a field-sourced job: what every dv_infer_cutouts* / dv_infer_fields* call gives
static PipeJob fields_job(const double* fields, int32_t F, int32_t nb, const int32_t* starts, uint64_t seed) {
  PipeJob j;
  j.fields = fields;
  j.F = F;
  j.nb = nb;
  j.starts = starts;
  j.seed = seed;
  return j;
}

// ---- one field (dv_infer_cutouts, _keep, _stream, _composite): the many-field call with M = 1 ------------------------------
static int infer_one_field(dv_model* m, const char* who, int64_t N, const PipeJob& j, const FieldsRequest& rq = {}) {
  if (!j.fields || !j.starts) return DV_E_INVALID;
  const int64_t field_ptr[2] = {0, N};
  return infer_fields_impl(m, who, 1, field_ptr, N, j, rq);
}

int dv_infer_cutouts(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                     uint64_t seed, float* loc, float* scale, float* mu, float* zstd, float* z) {
  PipeJob j = fields_job(field, F, nb, starts, seed);
  j.loc = loc;
  j.scale = scale;
  j.mu = mu;
  j.zstd = zstd;
  j.z = z;
  return infer_one_field(m, "dv_infer_cutouts", N, j);
}

int dv_infer_cutouts_keep(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                          uint64_t seed, float* loc, float* scale, double* cutouts) {
  if (!cutouts) return DV_E_INVALID;
  PipeJob j = fields_job(field, F, nb, starts, seed);
  j.loc = loc;
  j.scale = scale;
  j.cutouts = cutouts;
  return infer_one_field(m, "dv_infer_cutouts_keep", N, j);
}

int dv_infer_cutouts_stream(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                            uint64_t seed, dv_chunk_fn consumer, void* user) {
  if (!consumer) return DV_E_INVALID;
  PipeJob j = fields_job(field, F, nb, starts, seed);
  j.consumer = consumer;
  j.user = user;
  return infer_one_field(m, "dv_infer_cutouts_stream", N, j);
}

int dv_infer_cutouts_composite(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts,
                               const int32_t* places, int64_t N, uint64_t seed, double* mean_field, double* stddev_field,
                               double* residual_field, double* mse_center) {
  if (!places || !mean_field || !stddev_field) return DV_E_INVALID;
  FieldsRequest rq;
  rq.fields = FieldsOut{mean_field, stddev_field, residual_field, mse_center};
  rq.places = places;
  return infer_one_field(m, "dv_infer_cutouts_composite", N, fields_job(field, F, nb, starts, seed), rq);
}

// ---- many fields ------------------------------------------------------------------------------------------------------------
int dv_infer_fields(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                    const int64_t* field_ptr, int64_t N, uint64_t seed, float* loc, float* scale, float* mu, float* zstd,
                    float* z) {
  PipeJob j = fields_job(fields, F, nb, starts, seed);
  j.loc = loc;
  j.scale = scale;
  j.mu = mu;
  j.zstd = zstd;
  j.z = z;
  return infer_fields_impl(m, "dv_infer_fields", M, field_ptr, N, j, {});
}

int dv_infer_fields_keep(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                         const int64_t* field_ptr, int64_t N, uint64_t seed, float* loc, float* scale, float* mu,
                         float* zstd, float* z, double* cutouts) {
  if (!cutouts && N > 0) return DV_E_INVALID;
  PipeJob j = fields_job(fields, F, nb, starts, seed);
  j.loc = loc;
  j.scale = scale;
  j.mu = mu;
  j.zstd = zstd;
  j.z = z;
  j.cutouts = cutouts;
  return infer_fields_impl(m, "dv_infer_fields_keep", M, field_ptr, N, j, {});
}

int dv_infer_fields_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                              const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                              double* mean_fields, double* stddev_fields, double* residual_fields, double* mse_center) {
  if ((M > 0 && (!mean_fields || !stddev_fields)) || (N > 0 && !places)) return DV_E_INVALID;
  FieldsRequest rq;
  rq.fields = FieldsOut{mean_fields, stddev_fields, residual_fields, mse_center};
  rq.places = places;
  return infer_fields_impl(m, "dv_infer_fields_composite", M, field_ptr, N, fields_job(fields, F, nb, starts, seed), rq);
}

// ---- catalogue measurement as a stage of the many-field call -----------------------------------------------
// what every dv_infer_fields_measure* call takes, in the order of the C ABI (between seed and params the Monte-Carlo call
// has its two arguments; the outputs of an extra follow status)
struct CatalogueArgs {
  const double* fields;
  int32_t M, F, nb;
  const int32_t *starts, *places;
  const int64_t* field_ptr;
  int64_t N;
  uint64_t seed;
  const dv_measure_params* params;
  double *mean_fields, *stddev_fields, *residual_fields, *mse_center;   // all three fields null: the catalogue-only call
  double *flux, *flux_err, *shape;
  int32_t *iters, *status;
};

// the places of a catalogue-only call whose extra composites on the device all the same
static int seam_places_check(const char* who, const CatalogueArgs& a) {
  if (a.N > 0 && !a.places) {
    set_error("%s: places must be given (the catalogue-only form needs the placements too)", who);
    return DV_E_INVALID;
  }
  return DV_OK;
}

// rq: the extra of the call, filled in by its entry point; the catalogue, the result fields and the places are filled in here
static int infer_fields_measure_entry(const char* who, dv_model* m, const CatalogueArgs& a, FieldsRequest& rq) {
  if (!m || !a.params) return DV_E_INVALID;
  const dv_measure_params& par = *a.params;
  const int64_t N = a.N;
  DV_TRY(measure_check(who, m->A.H, a.nb, par.band, par.sigma0, par.tol, par.max_iter));
  if (rq.mc && rq.mc->nsamples < 1) {
    set_error("%s: %d Monte-Carlo samples asked for, at least 1 is needed", who, rq.mc->nsamples);
    return DV_E_INVALID;
  }
  if (rq.aper) {
    DV_TRY(aperture_check(who, m->A.H, a.nb, par.band, rq.aper->par));
    DV_TRY(aperture_rows_check(who, rq.aper->rows, rq.aper->par, true, N));
  }
  if (rq.aper_field) {
    DV_TRY(aperture_field_rows_check(who, rq.aper_field->rows, rq.aper->par, N));
    DV_TRY(seam_places_check(who, a));
  }
  if (rq.fit_flux) {
    DV_TRY(fitflux_check(who, m->A.H, a.nb, a.F, rq.fit_flux->par));
    DV_TRY(fitflux_rows_check(who, rq.fit_flux->rows, N, rq.fit_flux->weights != nullptr));
    if (rq.fit_flux->sky.q) DV_TRY(fitflux_sky_check(who, rq.fit_flux->sky_order, rq.fit_flux->sky, rq.fit_flux->rows,
                                                     rq.fit_flux->weights != nullptr));
    if (rq.fit_flux->nonneg.on) DV_TRY(fitflux_nonneg_check(who, rq.fit_flux->nonneg, rq.fit_flux->rows, N, rq.fit_flux->sky,
                                                            rq.fit_flux->weights != nullptr));
    if (rq.fit_flux->grouped() && !rq.fit_flux->weights && (rq.fit_flux->rows.chi2 || rq.fit_flux->rows.npix)) {
      set_error("%s: fit_chi2 and fit_npix are the outputs of the weighted fit: without weight_fields both must be NULL", who);
      return DV_E_INVALID;
    }
    DV_TRY(seam_places_check(who, a));
  }
  if (rq.moments) {
    DV_TRY(moments_field_rows_check(who, rq.moments->rows, N));
    DV_TRY(seam_places_check(who, a));
  }
  if (rq.regauss) {
    const RegaussOut& ro = *rq.regauss;
    DV_TRY(regauss_check(who, m->A.H, a.nb, par.band, ro.K, ro.ps, ro.psf_sigma0, par.tol, par.max_iter));
    if (!ro.psf || !ro.psf_shape || !ro.psf_aux || !ro.psf_iters || !ro.psf_status ||
        (N > 0 && (!ro.index || !ro.out || !ro.iters || !ro.status))) {
      set_error("%s: psf, psf_index, regauss, regauss_iters, regauss_status, psf_shape, psf_aux, psf_iters and psf_status must "
                "all be given", who);
      return DV_E_INVALID;
    }
  }
  if (N > 0 && (!a.flux || !a.flux_err || !a.shape || !a.iters || !a.status)) {
    set_error("%s: flux, flux_err, shape, iters and status must all be given", who);
    return DV_E_INVALID;
  }
  if (rq.mc) {
    const McState& st = rq.mc->st;
    if (N > 0 && (!st.flux_mean || !st.flux_std || !st.shape_mean || !st.shape_std || !st.n_ok)) {
      set_error("%s: the Monte-Carlo outputs flux_mean, flux_std, shape_mean, shape_std and n_ok must all be given", who);
      return DV_E_INVALID;
    }
    const int given = (st.sample_flux != nullptr) + (st.sample_shape != nullptr) + (st.sample_status != nullptr);
    if (given != 0 && given != 3) {
      set_error("%s: the per-sample outputs sample_flux, sample_shape and sample_status go together (all given or all null)", who);
      return DV_E_INVALID;
    }
  }
  const bool with_fields = a.mean_fields || a.stddev_fields || a.residual_fields;
  if (with_fields && ((a.M > 0 && (!a.mean_fields || !a.stddev_fields)) || (N > 0 && !a.places))) {
    set_error("%s: mean_fields, stddev_fields and places go together (residual_fields is optional beside them); the "
              "catalogue-only call passes all three fields as null", who);
    return DV_E_INVALID;
  }
  if (rq.blend && N > 0 && (!a.places || !rq.blend->blend || !rq.blend->npix)) {
    set_error("%s: places, blend and npix must all be given (the catalogue-only form needs the placements too)", who);
    return DV_E_INVALID;
  }
  rq.cat = MeasureOut{par, a.flux, a.flux_err, a.shape, a.iters, a.status};
  rq.places = a.places;
  if (with_fields)
    rq.fields = FieldsOut{a.mean_fields, a.stddev_fields, a.residual_fields, a.mse_center};
  else
    rq.cat->mse = a.mse_center;      // (no FieldsOut to carry it)
  PipeJob j = fields_job(a.fields, a.F, a.nb, a.starts, a.seed);
  if (rq.mc) {
    j.mc_samples = rq.mc->nsamples;
    j.mc_seed = rq.mc->seed;
  }
  return infer_fields_impl(m, who, a.M, a.field_ptr, N, j, rq);
}

int dv_infer_fields_measure(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                            const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                            const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                            double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                            int32_t* iters, int32_t* status) {
  FieldsRequest rq;
  return infer_fields_measure_entry("dv_infer_fields_measure", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- blendedness beside the catalogue: dv_infer_fields_measure plus the four weighted sums per galaxy; the
// placements are always needed
int dv_infer_fields_measure_blend(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                  const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                  const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                  double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                  int32_t* iters, int32_t* status, double* blend, int32_t* npix) {
  FieldsRequest rq;
  rq.blend = BlendOut{blend, npix};
  return infer_fields_measure_entry("dv_infer_fields_measure_blend", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- PSF-corrected shapes beside the catalogue: dv_infer_fields_measure plus the re-Gaussianized moments
int dv_infer_fields_measure_psf(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                int32_t* iters, int32_t* status, const double* psf, int32_t K, int32_t ps,
                                const int32_t* psf_index, double psf_sigma0, double* regauss, int32_t* regauss_iters,
                                int32_t* regauss_status, double* psf_shape, double* psf_aux, int32_t* psf_iters,
                                int32_t* psf_status) {
  FieldsRequest rq;
  rq.regauss = RegaussOut{psf, K, ps, psf_index, psf_sigma0, regauss, regauss_iters, regauss_status, psf_shape, psf_aux,
                          psf_iters, psf_status};
  return infer_fields_measure_entry("dv_infer_fields_measure_psf", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- aperture photometry beside the catalogue: dv_infer_fields_measure plus circular apertures, the Kron flux
// and radius and the flux radii of every stamp
int dv_infer_fields_measure_aper(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                 const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                 const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                 double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                 int32_t* iters, int32_t* status, const dv_aperture_params* aper, double* ap_flux,
                                 double* ap_flux_err, double* ap_area, double* flux_auto, double* flux_auto_err, double* kron,
                                 double* flux_rho, int32_t* aper_flags, int32_t* aper_status) {
  if (!m) return DV_E_INVALID;
  if (!aper) {
    set_error("dv_infer_fields_measure_aper: the aperture params must be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.aper = ApertureOut{aperture_params(*aper), ApertureRows{ap_flux, ap_flux_err, ap_area, flux_auto, flux_auto_err, kron,
                                                              flux_rho, aper_flags, aper_status}};
  return infer_fields_measure_entry("dv_infer_fields_measure_aper", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the same apertures on the observed field with the neighbours subtracted: dv_infer_fields_measure_aper plus
// the sums of w T and w D inside the field, taken at the completed-field seam
int dv_infer_fields_measure_aper_data(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb,
                                      const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                                      uint64_t seed, const dv_measure_params* params, double* mean_fields,
                                      double* stddev_fields, double* residual_fields, double* mse_center, double* flux,
                                      double* flux_err, double* shape, int32_t* iters, int32_t* status,
                                      const dv_aperture_params* aper, double* ap_flux, double* ap_flux_err, double* ap_area,
                                      double* flux_auto, double* flux_auto_err, double* kron, double* flux_rho,
                                      int32_t* aper_flags, int32_t* aper_status, double* ap_model_sum, double* ap_data_sum,
                                      double* ap_field_area, double* auto_model_sum, double* auto_data_sum,
                                      double* auto_field_area) {
  if (!m) return DV_E_INVALID;
  if (!aper) {
    set_error("dv_infer_fields_measure_aper_data: the aperture params must be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.aper = ApertureOut{aperture_params(*aper), ApertureRows{ap_flux, ap_flux_err, ap_area, flux_auto, flux_auto_err, kron,
                                                              flux_rho, aper_flags, aper_status}};
  rq.aper_field = ApertureFieldOut{ApertureFieldRows{ap_model_sum, ap_data_sum, ap_field_area, auto_model_sum, auto_data_sum,
                                                     auto_field_area}};
  return infer_fields_measure_entry("dv_infer_fields_measure_aper_data", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the simultaneous flux fit beside the catalogue: dv_infer_fields_measure plus, per galaxy and band, the
// amplitude of its mean stamp in the least-squares fit of all the mean stamps of its field to the source field, taken at the
// completed-field seam from the mean stamps the chunk loop has kept
int dv_infer_fields_measure_fit(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, double* fit_scale,
                                double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status) {
  if (!m) return DV_E_INVALID;
  if (!fit) {
    set_error("dv_infer_fields_measure_fit: the flux-fit params must be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fit_flux = FitFluxOut{FitFluxParams{fit->min_pivot, fit->scratch_bytes},
                           FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status}};
  return infer_fields_measure_entry("dv_infer_fields_measure_fit", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the same under per-pixel inverse-variance weights: dv_infer_fields_measure_fit plus the weight fields, laid
// out like the source fields and resident beside them, and the chi-square and pixel count of every galaxy and band
int dv_infer_fields_measure_fit_weighted(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb,
                                         const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                                         uint64_t seed, const dv_measure_params* params, double* mean_fields,
                                         double* stddev_fields, double* residual_fields, double* mse_center, double* flux,
                                         double* flux_err, double* shape, int32_t* iters, int32_t* status,
                                         const dv_fit_flux_params* fit, const double* weight_fields, double* fit_scale,
                                         double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status,
                                         double* fit_chi2, int32_t* fit_npix) {
  if (!m) return DV_E_INVALID;
  if (!fit) {
    set_error("dv_infer_fields_measure_fit_weighted: the flux-fit params must be given");
    return DV_E_INVALID;
  }
  if (!weight_fields) {
    set_error("dv_infer_fields_measure_fit_weighted: weight_fields must be given (dv_infer_fields_measure_fit is the unweighted fit)");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fit_flux = FitFluxOut{FitFluxParams{fit->min_pivot, fit->scratch_bytes},
                           FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields};
  return infer_fields_measure_entry("dv_infer_fields_measure_fit_weighted", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the adaptive moments on the observed field with the neighbours subtracted: dv_infer_fields_measure plus,
// per galaxy, the sums, the counting pixels and the moments of its child image D - T + P, taken at the completed-field seam from
// the mean stamps the chunk loop has kept; weight_fields may be NULL (no mask)
int dv_infer_fields_measure_moments_data(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                         const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                         const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                         double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                         int32_t* iters, int32_t* status, const double* weight_fields, double* flux_data,
                                         int32_t* npix_data, double* shape_data, int32_t* iters_data, int32_t* status_data) {
  FieldsRequest rq;
  rq.moments = MomentsFieldOut{MomentsFieldRows{flux_data, npix_data, shape_data, iters_data, status_data}, weight_fields};
  return infer_fields_measure_entry("dv_infer_fields_measure_moments_data", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the flux fit by blend groups: dv_infer_fields_measure_fit[_weighted] - weight_fields may be NULL, and
// fit_chi2 and fit_npix are NULL exactly then - without a limit per field, plus the group and the group size of every galaxy
int dv_infer_fields_measure_fit_groups(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                       const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                       const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                       double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                       int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                       double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status,
                                       double* fit_chi2, int32_t* fit_npix, int32_t* fit_group, int32_t* fit_group_size) {
  if (!m) return DV_E_INVALID;
  if (!fit) {
    set_error("dv_infer_fields_measure_fit_groups: the flux-fit params must be given");
    return DV_E_INVALID;
  }
  if (!fit_group || !fit_group_size) {
    set_error("dv_infer_fields_measure_fit_groups: fit_group and fit_group_size must all be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fit_flux = FitFluxOut{FitFluxParams{fit->min_pivot, fit->scratch_bytes},
                           FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields};
  rq.fit_flux->group = fit_group;
  rq.fit_flux->group_size = fit_group_size;
  return infer_fields_measure_entry("dv_infer_fields_measure_fit_groups", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the flux fit with a sky background fitted jointly: dv_infer_fields_measure_fit[_weighted] - weight_fields
// may be NULL, and fit_chi2 and fit_npix are NULL exactly then - plus the order of the sky and its per-field outputs
int dv_infer_fields_measure_fit_sky(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                    const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                    const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                    double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                    int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                    int32_t sky_order, double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj,
                                    int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef, double* sky_cov,
                                    int32_t* sky_status, int64_t* sky_npix) {
  if (!m) return DV_E_INVALID;
  if (!fit) {
    set_error("dv_infer_fields_measure_fit_sky: the flux-fit params must be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fit_flux = FitFluxOut{FitFluxParams{fit->min_pivot, fit->scratch_bytes},
                           FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight_fields,
                           sky_order, FitFluxSky{-1, sky_coef, sky_cov, sky_status, (long long*)sky_npix}};
  return infer_fields_measure_entry("dv_infer_fields_measure_fit_sky", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the non-negative flux fit: dv_infer_fields_measure_fit_sky - sky_order may be -1, no sky, and the four
// sky outputs are NULL exactly then - plus max_iter, three more galaxy rows and the two per-field outputs of the iteration
int dv_infer_fields_measure_fit_nonneg(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                       const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                       const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                       double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                       int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                       int32_t sky_order, int32_t max_iter, double* fit_scale, double* fit_var, double* fit_gram,
                                       double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef,
                                       double* sky_cov, int32_t* sky_status, int64_t* sky_npix, double* fit_scale_free,
                                       int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters, int32_t* nonneg_status) {
  if (!m) return DV_E_INVALID;
  if (!fit) {
    set_error("dv_infer_fields_measure_fit_nonneg: the flux-fit params must be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fit_flux = FitFluxOut{FitFluxParams{fit->min_pivot, fit->scratch_bytes},
                           FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix, fit_scale_free,
                                       fit_clamped, fit_dual},
                           weight_fields, sky_order,
                           FitFluxSky{sky_order == -1 ? 0 : -1, sky_coef, sky_cov, sky_status, (long long*)sky_npix},
                           FitFluxNonneg{true, max_iter, nonneg_iters, nonneg_status}};
  return infer_fields_measure_entry("dv_infer_fields_measure_fit_nonneg", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// ---- the Monte-Carlo catalogue beside it: dv_infer_fields_measure plus means and standard deviations of
// the measurement over nsamples stochastic decodes of every galaxy; no epistemic field, no eps_norm
int dv_infer_fields_measure_mc(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                               const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed,
                               int32_t nsamples, const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                               double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                               int32_t* iters, int32_t* status, double* flux_mean, double* flux_std, double* shape_mean,
                               double* shape_std, int32_t* n_ok, double* sample_flux, double* sample_shape,
                               int32_t* sample_status) {
  FieldsRequest rq;
  rq.mc = MeasureMcOut{McState{flux_mean, flux_std, shape_mean, shape_std, n_ok, sample_flux, sample_shape, sample_status},
                       nsamples, mc_seed};
  return infer_fields_measure_entry("dv_infer_fields_measure_mc", m,
                                    {fields, M, F, nb, starts, places, field_ptr, N, seed, params, mean_fields, stddev_fields,
                                     residual_fields, mse_center, flux, flux_err, shape, iters, status}, rq);
}

// the refusals of the two Monte-Carlo forms, before any GPU work
static int infer_fields_mc_check(dv_model* m, const char* who, int32_t nb, int32_t nsamples) {
  if (!m) return DV_E_INVALID;
  if (nsamples < 1) {
    set_error("%s: %d Monte-Carlo samples asked for, at least 1 is needed", who, nsamples);
    return DV_E_INVALID;
  }
  if (nb < 3 || m->A.C < 3) {
    set_error("%s: the normalised epistemic uncertainty is read from band 2, the stamps have %d bands", who,
              std::min<int>(nb, m->A.C));
    return DV_E_INVALID;
  }
  return DV_OK;
}

int dv_infer_fields_mc_keep(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                            const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed, int32_t nsamples,
                            float* loc, float* scale, double* cutouts, float* epistemic) {
  DV_TRY(infer_fields_mc_check(m, "dv_infer_fields_mc_keep", nb, nsamples));
  if (N > 0 && (!loc || !scale || !cutouts || !epistemic)) {
    set_error("dv_infer_fields_mc_keep: loc, scale, cutouts and epistemic must all be given");
    return DV_E_INVALID;
  }
  PipeJob j = fields_job(fields, F, nb, starts, seed);
  j.loc = loc;
  j.scale = scale;
  j.cutouts = cutouts;
  j.eps_out = epistemic;
  j.mc_samples = nsamples;
  j.mc_seed = mc_seed;
  return infer_fields_impl(m, "dv_infer_fields_mc_keep", M, field_ptr, N, j, {});
}

int dv_infer_fields_mc_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                 const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed,
                                 int32_t nsamples, double* mean_fields, double* stddev_fields, double* epistemic_fields,
                                 double* residual_fields, double* mse_center, double* eps_norm) {
  DV_TRY(infer_fields_mc_check(m, "dv_infer_fields_mc_composite", nb, nsamples));
  if ((M > 0 && (!mean_fields || !stddev_fields || !epistemic_fields)) || (N > 0 && (!eps_norm || !places))) {
    set_error("dv_infer_fields_mc_composite: mean_fields, stddev_fields, epistemic_fields, eps_norm and places must all be given");
    return DV_E_INVALID;
  }
  FieldsRequest rq;
  rq.fields = FieldsOut{mean_fields, stddev_fields, residual_fields, mse_center};
  rq.fields->epistemic = epistemic_fields;
  rq.fields->eps_norm = eps_norm;
  rq.places = places;
  PipeJob j = fields_job(fields, F, nb, starts, seed);
  j.mc_samples = nsamples;
  j.mc_seed = mc_seed;
  return infer_fields_impl(m, "dv_infer_fields_mc_composite", M, field_ptr, N, j, rq);
}

// ---- position fit and fractional placements in the many-field composite call -------------------------------
int dv_infer_fields_fit_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                  const double* dist, const int64_t* field_ptr, int64_t N, uint64_t seed, double bound,
                                  int32_t max_iter, double* shifts_inout, uint64_t mc_seed, int32_t nsamples,
                                  double* mean_fields, double* stddev_fields, double* epistemic_fields,
                                  double* residual_fields, double* mse_center, double* eps_norm, double* objective,
                                  int32_t* iters, int32_t* status) {
  const char* who = "dv_infer_fields_fit_composite";
  if (!m || N < 0 || N >= ((int64_t)1 << 31)) return DV_E_INVALID;
  if (nb < 3 || m->A.C < 3) {
    set_error("%s: the fit reads band 2, the stamps have %d bands", who, std::min<int>(nb, m->A.C));
    return DV_E_INVALID;
  }
  if (max_iter < 0 || !(bound >= 0.0) || bound > 1e6) {
    set_error("%s: bound must lie in 0 .. 1e6 and max_iter be >= 0 (got %g, %d)", who, bound, max_iter);
    return DV_E_INVALID;
  }
  if ((M > 0 && (!mean_fields || !stddev_fields)) || (N > 0 && (!dist || !shifts_inout || !objective || !iters || !status))) {
    set_error("%s: mean_fields, stddev_fields, dist, shifts_inout, objective, iters and status must all be given", who);
    return DV_E_INVALID;
  }
  const bool mc = nsamples != 0 || epistemic_fields || eps_norm;
  if (mc) {
    DV_TRY(infer_fields_mc_check(m, who, nb, nsamples));
    if ((M > 0 && !epistemic_fields) || (N > 0 && !eps_norm)) {
      set_error("%s: epistemic_fields and eps_norm go with nsamples > 0 (nsamples = 0 and both null: no Monte-Carlo stage)", who);
      return DV_E_INVALID;
    }
  }
  for (int64_t i = 0; i < 2 * N; ++i)
    if (!(dist[i] == floor(dist[i])) || dist[i] > 1e6 || dist[i] < -1e6) {
      set_error("%s: distance %g of galaxy %ld: the device path places at integer distances within +-1e6", who, dist[i],
                (long)(i / 2));
      return DV_E_INVALID;
    }
  FieldsRequest rq;
  FieldsOut& fo = rq.fields.emplace(FieldsOut{mean_fields, stddev_fields, residual_fields, mse_center});
  fo.epistemic = mc ? epistemic_fields : nullptr;
  fo.eps_norm = mc ? eps_norm : nullptr;
  fo.dist = dist;
  fo.bound = bound;
  fo.max_iter = max_iter;
  fo.shifts = shifts_inout;
  fo.objective = objective;
  fo.iters = iters;
  fo.status = status;
  PipeJob j = fields_job(fields, F, nb, starts, seed);
  if (mc) {
    j.mc_samples = nsamples;
    j.mc_seed = mc_seed;
  }
  return infer_fields_impl(m, who, M, field_ptr, N, j, rq);
}

// ---- resident field sets (dv_field_set_*) ---------------------------------------------------------------------
// M fields uploaded once; the working residuals, the final residuals and the predicted sums of an iterative deblending loop
// stay in HBM between its passes.  A pass is infer_fields_impl's composite job with the set's `work` stack as the source and
// the set's stacks as the sinks; nothing field-sized crosses the host link until dv_field_set_read.
static int field_set_live(const dv_field_set* fs, const char* who) {
  if (!fs) return DV_E_INVALID;
  if (!fs->open) {
    set_error("%s: the field set has been closed", who);
    return DV_E_STATE;
  }
  return DV_OK;
}

int dv_field_set_open(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, int32_t cumulative,
                      dv_field_set** out) {
  if (!m || !out || M < 0 || F < 1 || (M > 0 && !fields)) return DV_E_INVALID;
  *out = nullptr;
  const Arch& A = m->A;
  if (nb != A.C || A.H > F) {
    set_error("dv_field_set_open: the fields have %d bands and %d pixels, the network takes %d x %d x %d stamps", nb, F, A.H,
              A.H, A.C);
    return DV_E_INVALID;
  }
  if (M > 65535) {
    set_error("dv_field_set_open: %d fields, at most 65535 per set", M);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(m->ctx->device));
  const size_t felems = (size_t)F * F * nb, fb = felems * sizeof(double);
  const int nbuf = cumulative ? 4 : 6;
  const size_t nblk = (size_t)scene_field_mse_blocks((long)felems);
  const size_t need = (size_t)M * ((size_t)nbuf * fb + (nblk + 1) * sizeof(double));
  // what the passes allocate beside the set comes off the free memory first, as infer_fields_impl takes its pipeline
  // before its budget: the inference pipeline for the longest chunk a pass can make (unless the model already has it), the
  // detector's workspace for the fields of one launch (at most its 4 GiB cap; ~128 bytes per pixel), and 64 MiB for the
  // per-stamp tables (28 bytes per stamp)
  const size_t img = (size_t)m->Bc * A.H * A.H * A.C * sizeof(float);
  const size_t pipe_need = (m->pipe && m->pipe->cap >= m->Bc) ? 0 : 6 * img + 2 * (size_t)m->Bc * 3 * A.d * sizeof(float);
  const size_t det_need = std::min<size_t>((size_t)4 << 30, (size_t)M * F * F * 128);
  const size_t reserve = pipe_need + det_need + ((size_t)64 << 20);
  size_t budget = 0;
  DV_TRY(fields_budget(reserve, &budget));
  if (need > budget) {
    set_error("dv_field_set_open: %d resident %d-pixel fields with their %d buffers each need %zu bytes of device memory, "
              "%zu bytes are available for fields (a set is never split: open fewer fields per set)", M, F, nbuf, need, budget);
    return DV_E_NOMEM;
  }
  std::unique_ptr<dv_field_set> fs(new dv_field_set());
  fs->m = m;
  fs->M = M;
  fs->F = F;
  fs->nb = nb;
  fs->cumulative = cumulative != 0;
  fs->open = true;
  hipStream_t s = m->ctx->stream;
  StreamDrain drain(s);                       // a failure waits for the stream before the set's buffers go
  const size_t all = (size_t)M * felems;
  for (DevBuf<double>* b : {&fs->work, &fs->next, &fs->mean, &fs->stddev}) DV_TRY(b->alloc(all));
  if (!fs->cumulative)
    for (DevBuf<double>* b : {&fs->base, &fs->fin}) DV_TRY(b->alloc(all));
  DV_TRY(fs->mse_part.alloc((size_t)M * nblk));
  DV_TRY(fs->fmse.alloc((size_t)M));
  DV_TRY(fs->tab.fptr.alloc((size_t)M + 1));
  fs->fmse_h.assign((size_t)M, 0.0);
  if (M > 0) {
    DV_HIP(hipMemcpyAsync(fs->work, fields, (size_t)M * fb, hipMemcpyHostToDevice, s));
    DV_HIP(hipMemsetAsync(fs->mean, 0, (size_t)M * fb, s));
    DV_HIP(hipMemsetAsync(fs->stddev, 0, (size_t)M * fb, s));
    if (!fs->cumulative) {
      DV_HIP(hipMemcpyAsync(fs->base, fs->work, (size_t)M * fb, hipMemcpyDeviceToDevice, s));
      DV_HIP(hipMemcpyAsync(fs->fin, fs->work, (size_t)M * fb, hipMemcpyDeviceToDevice, s));
    }
    DV_HIP(hipStreamSynchronize(s));
  }
  drain.dismiss();
  m->field_sets.push_back(fs.get());
  *out = fs.release();
  return DV_OK;
}

int dv_field_set_close(dv_field_set* fs) {
  DV_TRY(field_set_live(fs, "dv_field_set_close"));
  (void)hipSetDevice(fs->m->ctx->device);
  (void)hipStreamSynchronize(fs->m->ctx->stream);
  field_set_release(fs);                      // the handle itself lives as long as its model: later calls find it closed
  return DV_OK;
}

int dv_field_set_detect(dv_field_set* fs, const uint8_t* active, const dv_detect_params* p, int64_t cap, int64_t* n_out,
                        int64_t* offsets, double* globalrms, int32_t* field, int32_t* parent, int32_t* npix, double* peak,
                        double* flux, double* x, double* y) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect"));
  if (!p || !n_out || !offsets || !globalrms) return DV_E_INVALID;
  const bool multi = !fs->dbands.empty();
  if (!multi && fs->nb < 3) {
    set_error("dv_field_set_detect: detection reads band 2, the fields have %d band(s)", fs->nb);
    return DV_E_INVALID;
  }
  std::vector<int32_t> act;
  for (int f = 0; f < fs->M; ++f)
    if (!active || active[f]) act.push_back(f);
  const int Ma = (int)act.size();
  std::vector<int64_t> off((size_t)Ma + 1, 0);
  std::vector<double> grms((size_t)std::max(Ma, 1), 0.0);
  DV_HIP(hipSetDevice(fs->m->ctx->device));
  DetectDevSrc src{fs->work, fs->nb, multi ? 0 : 2, act.data(), fs->dweights, fs->dplanes};
  // (the planes of either mode lie in the set: src carries them, the host pointers stay null)
  const DetectWeights wq{nullptr, fs->dnoise, fs->dfilter};
  const DetectBands mb{fs->dbands.data(), (int)fs->dbands.size(), fs->dbw.data(), nullptr, (bool)fs->dplanes, fs->dbnoise,
                       fs->dbfilter};
  *n_out = 0;
  // (7zb) the object columns land in the set's host arrays, the segmap of the active fields in seg_a
  DetectObjects oq{};
  std::vector<int32_t> seg_a;
  const size_t FF = (size_t)fs->F * fs->F;
  if (fs->dobj) {
    if (p->thresh < 0.0) {
      set_error("dv_field_set_detect: with the object columns on thresh must be >= 0 (got %g)", p->thresh);
      return DV_E_INVALID;
    }
    fs->do_n = -1;
    for (int e = 0; e < DET_OBJ_I; ++e) {
      fs->do_i[e].assign((size_t)std::max<int64_t>(cap, 0), 0);
      oq.icol[e] = fs->do_i[e].data();
    }
    for (int e = 0; e < DET_OBJ_D; ++e) {
      fs->do_d[e].assign((size_t)std::max<int64_t>(cap, 0), 0.0);
      oq.dcol[e] = fs->do_d[e].data();
    }
    if (fs->dseg) {
      seg_a.assign(std::max<size_t>((size_t)Ma * FF, 1), 0);
      oq.segmap_h = seg_a.data();
    }
  }
  // (7zc) the clean columns land in the set's host arrays, n_raw of the active fields in nraw_a
  DetectClean cq{};
  std::vector<int64_t> nraw_a;
  if (fs->dclean) {
    DV_TRY(detect_clean_check("dv_field_set_detect", true, fs->dclean_param, p));
    fs->dc_n = -1;
    fs->dc_nmerged.assign((size_t)std::max<int64_t>(cap, 0), 0);
    fs->dc_mthresh.assign((size_t)std::max<int64_t>(cap, 0), 0.0);
    nraw_a.assign((size_t)std::max(Ma, 1), 0);
    cq = DetectClean{fs->dclean_param, fs->dc_nmerged.data(), fs->dc_mthresh.data(), nraw_a.data()};
  }
  if (Ma > 0) {
    DetectRequest rq{nullptr, 0, Ma, fs->F, fs->F, p, &src};
    rq.weights = (!multi && fs->dweights) ? &wq : nullptr; rq.bands = multi ? &mb : nullptr; rq.objects = fs->dobj ? &oq : nullptr;
    rq.clean = fs->dclean ? &cq : nullptr;
    rq.cat = DetectCatalog{cap, n_out, off.data(), grms.data(), field, parent, npix, peak, flux, x, y};
    DV_TRY(scene_detect(rq, fs->m->ctx->stream));
  }
  if (fs->dobj) {
    if (*n_out <= cap) fs->do_n = *n_out;
    if (fs->dseg) {
      fs->do_seg.assign((size_t)fs->M * FF, 0);
      for (int a = 0; a < Ma; ++a)
        std::copy(seg_a.begin() + (size_t)a * FF, seg_a.begin() + (size_t)(a + 1) * FF, fs->do_seg.begin() + (size_t)act[a] * FF);
    }
  }
  if (fs->dclean) {
    if (*n_out <= cap) fs->dc_n = *n_out;
    fs->dc_nraw.assign((size_t)fs->M, 0);
    for (int a = 0; a < Ma; ++a) fs->dc_nraw[act[a]] = nraw_a[a];
  }
  // the catalogue of the active fields in the numbering of the set: an inactive field has an empty range
  offsets[0] = 0;
  int a = 0;
  for (int f = 0; f < fs->M; ++f) {
    const bool on = a < Ma && act[a] == f;
    offsets[f + 1] = offsets[f] + (on ? off[a + 1] - off[a] : 0);
    globalrms[f] = on ? grms[a] : 0.0;
    if (on) ++a;
  }
  if (*n_out <= cap)
    for (int64_t i = 0; i < *n_out; ++i) field[i] = act[field[i]];
  return DV_OK;
}

int dv_field_set_detect_objects(dv_field_set* fs, int32_t on, int32_t segmap_on) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_objects"));
  fs->dobj = on != 0;
  fs->dseg = on != 0 && segmap_on != 0;
  fs->do_n = -1;
  for (auto& v : fs->do_i) std::vector<int32_t>().swap(v);
  for (auto& v : fs->do_d) std::vector<double>().swap(v);
  std::vector<int32_t>().swap(fs->do_seg);
  return DV_OK;
}

int dv_field_set_detect_objects_read(dv_field_set* fs, int64_t n_expected, const dv_detect_objects* out) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_objects_read"));
  if (!out) return DV_E_INVALID;
  if (!fs->dobj) {
    set_error("dv_field_set_detect_objects_read: the object columns are off (dv_field_set_detect_objects)");
    return DV_E_INVALID;
  }
  if (fs->do_n < 0) {
    set_error("dv_field_set_detect_objects_read: no detection is kept (none since the switch went on, or its catalogue did not "
              "fit its cap)");
    return DV_E_INVALID;
  }
  if (n_expected != fs->do_n) {
    set_error("dv_field_set_detect_objects_read: %lld rows expected, the last detection has %lld", (long long)n_expected,
              (long long)fs->do_n);
    return DV_E_INVALID;
  }
  if (out->segmap && !fs->dseg) {
    set_error("dv_field_set_detect_objects_read: the segmap was not asked for (dv_field_set_detect_objects)");
    return DV_E_INVALID;
  }
  const DetectObjects o = detect_objects_of(out);
  const size_t n = (size_t)fs->do_n;
  for (int e = 0; e < DET_OBJ_I; ++e)
    if (o.icol[e]) std::copy(fs->do_i[e].begin(), fs->do_i[e].begin() + n, o.icol[e]);
  for (int e = 0; e < DET_OBJ_D; ++e)
    if (o.dcol[e]) std::copy(fs->do_d[e].begin(), fs->do_d[e].begin() + n, o.dcol[e]);
  if (o.segmap_h) std::copy(fs->do_seg.begin(), fs->do_seg.end(), o.segmap_h);
  return DV_OK;
}

int dv_field_set_detect_clean(dv_field_set* fs, int32_t on, double clean_param) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_clean"));
  if (on != 0 && (!std::isfinite(clean_param) || !(clean_param > 0.0))) {
    set_error("dv_field_set_detect_clean: clean_param must be finite and > 0 (got %g)", clean_param);
    return DV_E_INVALID;
  }
  fs->dclean = on != 0;
  fs->dclean_param = on != 0 ? clean_param : 1.0;
  fs->dc_n = -1;
  std::vector<int32_t>().swap(fs->dc_nmerged);
  std::vector<double>().swap(fs->dc_mthresh);
  std::vector<int64_t>().swap(fs->dc_nraw);
  return DV_OK;
}

int dv_field_set_detect_clean_read(dv_field_set* fs, int64_t n_expected, int32_t* nmerged, double* mthresh, int64_t* n_raw) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_clean_read"));
  if (!fs->dclean) {
    set_error("dv_field_set_detect_clean_read: the cleaning pass is off (dv_field_set_detect_clean)");
    return DV_E_INVALID;
  }
  if (fs->dc_n < 0) {
    set_error("dv_field_set_detect_clean_read: no detection is kept (none since the switch went on, or its catalogue did not "
              "fit its cap)");
    return DV_E_INVALID;
  }
  if (n_expected != fs->dc_n) {
    set_error("dv_field_set_detect_clean_read: %lld rows expected, the last detection has %lld", (long long)n_expected,
              (long long)fs->dc_n);
    return DV_E_INVALID;
  }
  const size_t n = (size_t)fs->dc_n;
  if (nmerged) std::copy(fs->dc_nmerged.begin(), fs->dc_nmerged.begin() + n, nmerged);
  if (mthresh) std::copy(fs->dc_mthresh.begin(), fs->dc_mthresh.begin() + n, mthresh);
  if (n_raw) std::copy(fs->dc_nraw.begin(), fs->dc_nraw.end(), n_raw);
  return DV_OK;
}

int dv_field_set_detect_bands(dv_field_set* fs, const int32_t* bands, int32_t k, const double* band_weights,
                              const double* planes, int32_t noise, int32_t filter) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_bands"));
  DV_HIP(hipSetDevice(fs->m->ctx->device));
  hipStream_t s = fs->m->ctx->stream;
  if (k == 0) {                                 // drop the selection: dv_field_set_detect reads band 2 again
    DV_HIP(hipStreamSynchronize(s));
    fs->dplanes.reset();
    fs->dbands.clear();
    fs->dbw.clear();
    return DV_OK;
  }
  if (fs->dweights) {
    set_error("dv_field_set_detect_bands: the set holds single-band planes of dv_field_set_detect_weights; drop them first");
    return DV_E_INVALID;
  }
  DV_TRY(detect_bands_check("dv_field_set_detect_bands", bands, k, band_weights, fs->nb, planes ? noise : 0, filter));
  const size_t n = (size_t)fs->M * fs->F * fs->F * (size_t)k;
  if (!planes) {
    DV_HIP(hipStreamSynchronize(s));
    fs->dplanes.reset();
  } else {
    if (!fs->dplanes || fs->dbands.size() != (size_t)k) {
      // counted like the set itself: against free memory less the detector's workspace and the per-stamp tables (planes of
      // another k that the set holds are not counted as free: a refusal leaves them in place)
      const size_t reserve = std::min<size_t>((size_t)4 << 30, (size_t)fs->M * fs->F * fs->F * 128) + ((size_t)64 << 20);
      size_t budget = 0;
      DV_TRY(fields_budget(reserve, &budget));
      if (n * sizeof(double) > budget) {
        set_error("dv_field_set_detect_bands: the %d planes of %d %d-pixel fields need %zu bytes of device memory, %zu bytes "
                  "are available", k, fs->M, fs->F, n * sizeof(double), budget);
        return DV_E_NOMEM;
      }
      DV_HIP(hipStreamSynchronize(s));
      fs->dplanes.reset();
      fs->dbands.clear();
      fs->dbw.clear();
      DV_TRY(fs->dplanes.alloc(std::max<size_t>(n, 1)));
    }
    if (n > 0) {
      DV_HIP(hipMemcpyAsync(fs->dplanes, planes, n * sizeof(double), hipMemcpyHostToDevice, s));
      DV_HIP(hipStreamSynchronize(s));
    }
  }
  fs->dbands.assign(bands, bands + k);
  fs->dbw.assign((size_t)k, 1.0);
  if (band_weights) fs->dbw.assign(band_weights, band_weights + k);
  fs->dbnoise = noise;
  fs->dbfilter = filter;
  return DV_OK;
}

int dv_field_set_detect_weights(dv_field_set* fs, const double* weights, int32_t noise, int32_t filter) {
  DV_TRY(field_set_live(fs, "dv_field_set_detect_weights"));
  DV_HIP(hipSetDevice(fs->m->ctx->device));
  hipStream_t s = fs->m->ctx->stream;
  if (weights && !fs->dbands.empty()) {
    set_error("dv_field_set_detect_weights: the set holds a band selection of dv_field_set_detect_bands; drop it first");
    return DV_E_INVALID;
  }
  if (!weights) {                               // drop the planes: dv_field_set_detect is the unweighted call again
    DV_HIP(hipStreamSynchronize(s));
    fs->dweights.reset();
    return DV_OK;
  }
  if ((noise != DV_DETECT_NOISE_ABSOLUTE && noise != DV_DETECT_NOISE_RELATIVE) ||
      (filter != DV_DETECT_FILTER_CONV && filter != DV_DETECT_FILTER_MATCHED)) {
    set_error("dv_field_set_detect_weights: noise must be 0 (absolute) or 1 (relative) and filter 0 (conv) or 1 (matched), "
              "got %d, %d", noise, filter);
    return DV_E_INVALID;
  }
  const size_t n = (size_t)fs->M * fs->F * fs->F;
  if (!fs->dweights) {
    // counted like the set itself: against free memory less the detector's workspace and the per-stamp tables
    const size_t reserve = std::min<size_t>((size_t)4 << 30, n * 128) + ((size_t)64 << 20);
    size_t budget = 0;
    DV_TRY(fields_budget(reserve, &budget));
    if (n * sizeof(double) > budget) {
      set_error("dv_field_set_detect_weights: the weight planes of %d %d-pixel fields need %zu bytes of device memory, %zu "
                "bytes are available", fs->M, fs->F, n * sizeof(double), budget);
      return DV_E_NOMEM;
    }
    DV_TRY(fs->dweights.alloc(std::max<size_t>(n, 1)));
  }
  if (n > 0) {
    DV_HIP(hipMemcpyAsync(fs->dweights, weights, n * sizeof(double), hipMemcpyHostToDevice, s));
    DV_HIP(hipStreamSynchronize(s));
  }
  fs->dnoise = noise;
  fs->dfilter = filter;
  return DV_OK;
}

// mo: dv_field_set_pass_measure - the measurement of 7j behind every chunk's forward pass; bo beside it: the child sums of 7l
// behind that, and the pass's rows join the set's resident rows.  Without mo this is dv_field_set_pass as it
// was: the same launches in the same order.
static int field_set_pass_impl(dv_field_set* fs, const char* who, const int32_t* starts, const int32_t* places,
                               const int64_t* field_ptr, int64_t N, uint64_t seed, double* mse_center, double* field_mse,
                               const MeasureOut* mo = nullptr, const BlendOut* bo = nullptr) {
  DV_TRY(field_set_live(fs, who));
  dv_model* m = fs->m;
  const int M = fs->M, F = fs->F, nb = fs->nb;
  if (N > 0 && (!places || !mse_center || !field_mse)) {
    set_error("%s: places, mse_center and field_mse must all be given", who);
    return DV_E_INVALID;
  }
  if (mo) {
    DV_TRY(measure_check(who, m->A.H, nb, mo->par.band, mo->par.sigma0, mo->par.tol, mo->par.max_iter));
    if (N > 0 && (!mo->flux || !mo->flux_err || !mo->shape || !mo->iters || !mo->status)) {
      set_error("%s: flux, flux_err, shape, iters and status must all be given", who);
      return DV_E_INVALID;
    }
    if (bo && N >= 0 && (int64_t)fs->nrows + N >= ((int64_t)1 << 31)) {
      set_error("%s: %zu resident rows and %ld more, at most 2^31 - 1 per set", who, fs->nrows, (long)N);
      return DV_E_INVALID;
    }
  }
  std::vector<int32_t> sfield;
  std::vector<int> fptr32;
  DV_TRY(fields_tables(m, who, M, field_ptr, N, F, nb, starts, places, sfield, fptr32));
  if (N == 0) return DV_OK;
  TinyCall tiny(m, N);
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const int chunk = infer_chunk(m, N);
  InferPipe* pipe = nullptr;
  DV_TRY(pipe_get(m, chunk, &pipe, false));
  const long felems = (long)F * F * nb;
  StreamDrain drain(s, pipe->s_in, pipe->s_out);     // on a failure nothing may still read the set's tables
  StampTables& tab = fs->tab;                        // they grow to the largest pass so far
  DV_TRY(tab.upload(N, M, starts, places, sfield.data(), fptr32.data(), true, 1024, s));
  // the new working residual of every field that has stamps starts from the buffer the mode says
  DV_TRY(launch_scene_fields_copy(fs->next, fs->cumulative ? fs->work : fs->base, tab.fptr, M, felems, s));
  DV_HIP(hipStreamSynchronize(s));                   // the gather and the sinks run on the pipeline's copy streams
  PipeJob j;
  j.fields_d = fs->work;
  j.F = F;
  j.nb = nb;
  j.starts = starts;
  j.starts_d = tab.starts;
  j.sfield = sfield.data();
  j.sfield_d = tab.sfield;
  j.fptr_d = tab.fptr;
  j.N = N;
  j.chunk = chunk;
  j.seed = seed;
  j.sinks.mean_f = fs->mean;
  j.sinks.std_f = fs->stddev;
  j.sinks.res_f = fs->next;
  j.sinks.res2_f = fs->cumulative ? nullptr : fs->fin.get();
  j.sinks.places_d = tab.places;
  j.sinks.mse = tab.mse;
  const size_t n = (size_t)N, row0 = fs->nrows;
  if (mo) {
    // the pass measures into the tail of the resident rows (pipeline row r is resident row row0 + r); they are kept, and
    // the placements and fields set beside them, only if the pass took child sums and ran to its end
    DV_TRY(fs->rows_reserve(row0 + n, s));
    for (DevBuf<double>* b : {&fs->cflux, &fs->cferr}) DV_TRY(b->ensure(n * nb));
    DV_TRY(fs->citers.ensure(n));
    j.ms.flux = fs->cflux;
    j.ms.ferr = fs->cferr;
    j.ms.shape = fs->rshape.get() + row0 * 5;
    j.ms.iters = fs->citers;
    j.ms.status = fs->rstatus.get() + row0;
    j.ms.band = mo->par.band;
    j.ms.max_iter = mo->par.max_iter;
    j.ms.sigma0 = mo->par.sigma0;
    j.ms.tol = mo->par.tol;
    if (bo) {
      DV_TRY(fs->cblend.ensure(n * 4));
      DV_TRY(fs->cnpix.ensure(n));
      j.bl.blend = fs->cblend;
      j.bl.npix = fs->cnpix;
      if (fs->keep) {                                  // (7v: the pass's mean stamps, behind every chunk's measurement)
        const size_t stamp = (size_t)m->A.H * m->A.H * nb;
        DV_TRY(fs->stamps_reserve(row0 + n, stamp, s));
        j.ff.store = fs->rstamps.get() + row0 * stamp;
      }
    }
  }
  DV_TRY(infer_pipelined(m, j));
  // field_mse of the working residual against its successor, then the successor takes its place (fields with stamps only)
  DV_TRY(launch_scene_field_mse(fs->work, fs->next, tab.fptr, M, felems, fs->mse_part, fs->fmse, s));
  DV_TRY(launch_scene_fields_copy(fs->work, fs->next, tab.fptr, M, felems, s));
  std::vector<double>& fm = fs->fmse_h;
  DV_HIP(hipMemcpyAsync(mse_center, tab.mse, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(fm.data(), fs->fmse, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
  if (mo) {                                          // the catalogue's columns, as a view of the pass's rows (the set owns them)
    CatRows d{j.ms.flux, j.ms.ferr, j.ms.shape, j.ms.iters, j.ms.status};
    Rows view;
    catalogue_columns(view, d, CatRows{mo->flux, mo->flux_err, mo->shape, mo->iters, mo->status}, nb, true);
    DV_TRY(view.download(0, N, s));
  }
  if (bo) {
    // {W, A}: the first two of the four doubles the child kernel's rows have
    DV_HIP(hipMemcpy2DAsync(bo->blend, 2 * sizeof(double), fs->cblend, 4 * sizeof(double), 2 * sizeof(double), n,
                            hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(bo->npix, fs->cnpix, n * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(fs->rplaces.get() + row0 * 2, tab.places, n * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
    DV_HIP(hipMemcpyAsync(fs->rfield.get() + row0, tab.sfield, n * sizeof(int), hipMemcpyDeviceToDevice, s));
  }
  DV_HIP(hipStreamSynchronize(s));
  for (int f = 0; f < M; ++f)
    if (fptr32[f + 1] > fptr32[f]) field_mse[f] = fm[f];
  if (bo) fs->nrows = row0 + n;
  if (bo && fs->keep) {
    fs->pass_fptr.push_back(fptr32);
    fs->places_h.insert(fs->places_h.end(), places, places + 2 * n);
  }
  drain.dismiss();
  return prof_flush(m);
}

int dv_field_set_pass(dv_field_set* fs, const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                      uint64_t seed, double* mse_center, double* field_mse) {
  return field_set_pass_impl(fs, "dv_field_set_pass", starts, places, field_ptr, N, seed, mse_center, field_mse);
}

// ---- the catalogue of the iterative loop -----------------------------------------------------------------------
int dv_field_set_pass_measure(dv_field_set* fs, const int32_t* starts, const int32_t* places, const int64_t* field_ptr,
                              int64_t N, uint64_t seed, const dv_measure_params* params, double* mse_center, double* field_mse,
                              double* flux, double* flux_err, double* shape, int32_t* iters, int32_t* status, double* child,
                              int32_t* npix) {
  const char* who = "dv_field_set_pass_measure";
  DV_TRY(field_set_live(fs, who));
  if (!params) {
    set_error("%s: params must be given", who);
    return DV_E_INVALID;
  }
  if ((child == nullptr) != (npix == nullptr)) {
    set_error("%s: child and npix go together (both null: no child sums are taken and no resident rows are kept)", who);
    return DV_E_INVALID;
  }
  MeasureOut mo;
  mo.par = *params;
  mo.flux = flux;
  mo.flux_err = flux_err;
  mo.shape = shape;
  mo.iters = iters;
  mo.status = status;
  BlendOut bo;
  bo.blend = child;
  bo.npix = npix;
  return field_set_pass_impl(fs, who, starts, places, field_ptr, N, seed, mse_center, field_mse, &mo, child ? &bo : nullptr);
}

int dv_field_set_blend(dv_field_set* fs, int32_t band, int64_t n_expected, double* sums) {
  const char* who = "dv_field_set_blend";
  DV_TRY(field_set_live(fs, who));
  DV_TRY(blend_check(who, fs->m->A.H, fs->nb, band));
  if (n_expected != (int64_t)fs->nrows) {
    set_error("%s: %ld rows expected, the set holds %zu resident rows", who, (long)n_expected, fs->nrows);
    return DV_E_INVALID;
  }
  if (fs->nrows > 0 && !sums) {
    set_error("%s: sums must be given", who);
    return DV_E_INVALID;
  }
  if (fs->nrows == 0) return DV_OK;
  DV_HIP(hipSetDevice(fs->m->ctx->device));
  hipStream_t s = fs->m->ctx->stream;
  StreamDrain drain(s);
  const size_t n = fs->nrows;
  DV_TRY(fs->rsums.ensure(n * 4));
  DV_TRY(launch_blend_set(fs->rshape, fs->rstatus, fs->rplaces, fs->rfield, (int)n, fs->m->A.H, fs->nb, band, fs->F, fs->mean,
                          fs->cumulative ? nullptr : fs->base.get(), (fs->cumulative ? fs->work : fs->fin).get(), fs->rsums,
                          s));
  DV_HIP(hipMemcpyAsync(sums, fs->rsums, n * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  drain.dismiss();
  return DV_OK;
}

// ---- the joint flux fit of all passes of the iterative loop ------------------------------------------------------
int dv_field_set_keep_stamps(dv_field_set* fs, int32_t on) {
  const char* who = "dv_field_set_keep_stamps";
  DV_TRY(field_set_live(fs, who));
  if (fs->nrows > 0) {
    set_error("%s: the set holds %zu resident rows whose stamps %s: the switch is set before the first measured pass", who,
              fs->nrows, fs->keep ? "are kept" : "are gone");
    return DV_E_STATE;
  }
  fs->keep = on != 0;
  return DV_OK;
}

// The two calls below are wrappers of field_set_fit_flux (fitflux.hip), which has every refusal behind these: the set's state
// here, then what the call was given.
static int field_set_fit_ready(const dv_field_set* fs, const char* who, const dv_fit_flux_params* params, int64_t n_expected) {
  DV_TRY(field_set_live(fs, who));
  if (!fs->keep) {
    set_error("%s: the set keeps no stamps: dv_field_set_keep_stamps(set, 1) comes before the first measured pass", who);
    return DV_E_STATE;
  }
  if (!params) {
    set_error("%s: params must be given", who);
    return DV_E_INVALID;
  }
  if (n_expected != (int64_t)fs->nrows) {
    set_error("%s: %ld rows expected, the set holds %zu resident rows", who, (long)n_expected, fs->nrows);
    return DV_E_INVALID;
  }
  return DV_OK;
}

static ResidentRows field_set_resident(const dv_field_set* fs) {
  return ResidentRows{fs->rstamps.get(), fs->rplaces.get(), fs->rfield.get(), fs->base.get(), fs->places_h.data(), fs->pass_fptr,
                      fs->nrows, fs->M, fs->F, fs->nb, fs->m->A.H};
}

int dv_field_set_fit_flux(dv_field_set* fs, int64_t n_expected, const double* data, const double* weight, int32_t sky_order,
                          int32_t nonneg, const dv_fit_flux_params* params, int32_t nonneg_max_iter, double* fit_scale,
                          double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status, double* fit_chi2,
                          int32_t* fit_npix, double* sky_coef, double* sky_cov, int32_t* sky_status, int64_t* sky_npix,
                          double* fit_scale_free, int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters,
                          int32_t* nonneg_status) {
  const char* who = "dv_field_set_fit_flux";
  DV_TRY(field_set_fit_ready(fs, who, params, n_expected));
  if (sky_order < -1 || sky_order > 1) {
    set_error("%s: sky_order must be -1 (no sky), 0 (a constant) or 1 (a plane), got %d", who, sky_order);
    return DV_E_INVALID;
  }
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix, fit_scale_free, fit_clamped,
                            fit_dual},
                weight, sky_order,
                FitFluxSky{sky_order == -1 ? 0 : -1, sky_coef, sky_cov, sky_status, (long long*)sky_npix},
                FitFluxNonneg{nonneg != 0, nonneg_max_iter, nonneg_iters, nonneg_status}};
  rq.who = who;
  return field_set_fit_flux(field_set_resident(fs), data, rq, fs->m->ctx->device, fs->m->ctx->stream);
}

// the same by blend groups, in place on the stamp store
int dv_field_set_fit_flux_groups(dv_field_set* fs, int64_t n_expected, const double* data, const double* weight,
                                 const dv_fit_flux_params* params, double* fit_scale, double* fit_var, double* fit_gram,
                                 double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, int32_t* fit_group,
                                 int32_t* fit_group_size) {
  const char* who = "dv_field_set_fit_flux_groups";
  DV_TRY(field_set_fit_ready(fs, who, params, n_expected));
  FitFluxOut rq{FitFluxParams{params->min_pivot, params->scratch_bytes},
                FitFluxRows{fit_scale, fit_var, fit_gram, fit_proj, fit_status, fit_chi2, fit_npix}, weight};
  rq.group = fit_group;
  rq.group_size = fit_group_size;
  rq.by_groups = true;                                  // (group rows that are missing are refused by name, in their turn)
  rq.who = who;
  return field_set_fit_flux(field_set_resident(fs), data, rq, fs->m->ctx->device, fs->m->ctx->stream);
}

int dv_field_set_read(dv_field_set* fs, int32_t which, double* out) {
  DV_TRY(field_set_live(fs, "dv_field_set_read"));
  const double* src = which == DV_FIELD_SET_WORK ? fs->work.get()
                      : which == DV_FIELD_SET_FINAL ? (fs->cumulative ? fs->work : fs->fin).get()
                      : which == DV_FIELD_SET_MEAN ? fs->mean.get()
                      : which == DV_FIELD_SET_STDDEV ? fs->stddev.get() : nullptr;
  if (!src || (fs->M > 0 && !out)) {
    set_error("dv_field_set_read: which = %d, expected DV_FIELD_SET_WORK, _FINAL, _MEAN or _STDDEV", which);
    return DV_E_INVALID;
  }
  if (fs->M == 0) return DV_OK;
  DV_HIP(hipSetDevice(fs->m->ctx->device));
  hipStream_t s = fs->m->ctx->stream;
  DV_HIP(hipMemcpyAsync(out, src, (size_t)fs->M * fs->F * fs->F * fs->nb * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  return DV_OK;
}

int dv_infer_mc(dv_model* m, const float* x, int64_t N, int32_t nsamples, uint64_t seed, float* mean_out,
                float* std_out) {
  if (!m || !x || N < 0 || nsamples < 1 || (!mean_out && !std_out)) return DV_E_INVALID;
  const Arch& A = m->A;
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  // running statistics live in the two gradient ping-pong buffers (unused during inference)
  float* mean = m->gA;
  float* m2 = m->gB;
  for (int64_t o = 0; o < N; o += m->Bc) {
    int nb = (int)std::min<int64_t>(m->Bc, N - o);
    DV_TRY(stage_host_batch(m, x + o * stamp, nb));
    if (m->normalise) DV_TRY(launch_normalise(m->stage_x, (long)nb * stamp, false, s));
    DV_TRY(bn_prepare(m, m->stage_x, nullptr, 0, nb, nb, false, false));
    DV_TRY(encoder_forward(m, m->stage_x, nullptr, 0, nb, false));           // once per chunk
    DV_TRY(mc_decode_stats(m, nb, nsamples, seed, (unsigned)o));   // nsamples decodes: mean in gA, std in gB
    if (mean_out)
      DV_HIP(hipMemcpyAsync(mean_out + o * stamp, mean, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    if (std_out) DV_HIP(hipMemcpyAsync(std_out + o * stamp, m2, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
    m->lastB = nb;
  }
  return prof_flush(m);
}

int dv_encode(dv_model* m, const float* x, int64_t N, float* t) {
  if (!m || !x || !t || N < 0) return DV_E_INVALID;
  const Arch& A = m->A;
  TinyCall tiny(m, N);
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  for (int64_t o = 0; o < N; o += m->Bc) {
    int nb = (int)std::min<int64_t>(m->Bc, N - o);
    DV_TRY(stage_host_batch(m, x + o * stamp, nb));
    DV_TRY(bn_prepare(m, m->stage_x, nullptr, 0, nb, nb, false, false));
    DV_TRY(encoder_forward(m, m->stage_x, nullptr, 0, nb, false));
    DV_TRY(copy_rows(t + o * A.tw, A.tw, m->t, A.twp, A.tw, nb, hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
  }
  return prof_flush(m);
}

int dv_decode(dv_model* m, const float* z, int64_t N, float* loc, float* scale) {
  if (!m || !z || N < 0) return DV_E_INVALID;
  const Arch& A = m->A;
  TinyCall tiny(m, N);
  DV_HIP(hipSetDevice(m->ctx->device));
  hipStream_t s = m->ctx->stream;
  const size_t stamp = (size_t)A.H * A.H * A.C;
  for (int64_t o = 0; o < N; o += m->Bc) {
    int nb = (int)std::min<int64_t>(m->Bc, N - o);
    DV_TRY(copy_rows(m->z, A.dp, z + o * A.d, A.d, A.d, nb, hipMemcpyHostToDevice, s));   // (the pad columns stay zero)
    DV_TRY(forward_all(m, nullptr, nullptr, nullptr, 0, nb, nb, false, false, false, nullptr, 0, 0u, 0u, false, false,
                       true, /*run_encoder=*/false));
    if (loc) DV_HIP(hipMemcpyAsync(loc + o * stamp, m->loc, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    if (scale)
      DV_HIP(hipMemcpyAsync(scale + o * stamp, m->scale, nb * stamp * sizeof(float), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));
  }
  return prof_flush(m);
}

int dv_model_get_activation(dv_model* m, const char* name, float* host, size_t nbytes) {
  if (!m || !name || !host) return DV_E_INVALID;
  const Arch& A = m->A;
  const size_t B = (size_t)m->lastB;
  const float* src = nullptr;
  size_t elems = 0;
  std::string n(name);
  if (n == "t" || n == "z" || n == "eps") {        // rows of tw / d values, stored with the padded strides twp / dp
    const size_t w = n == "t" ? A.tw : A.d, ld = n == "t" ? A.twp : A.dp;
    src = n == "t" ? m->t : n == "z" ? m->z : m->eps;
    if (nbytes != B * w * sizeof(float)) {
      set_error("activation %s holds %zu bytes, caller passed %zu", name, B * w * sizeof(float), nbytes);
      return DV_E_INVALID;
    }
    DV_HIP(hipSetDevice(m->ctx->device));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
    if (B) DV_HIP(hipMemcpy2D(host, w * sizeof(float), src, ld * sizeof(float), w * sizeof(float), B, hipMemcpyDeviceToHost));
    return DV_OK;
  }
  else if (n == "kl") { src = m->kl; elems = B; }
  else if (n == "dec_ah") { src = m->dec_ah; elems = B * A.dec_hidden; }       // PReLU output of the decoder's hidden Dense
  else if (n == "dec_uh") { src = m->dec_uh; elems = B * A.dec_hidden; }       // ... and its pre-activation
  else if (n == "d_t" && m->bf.on) { src = m->bf.trunk[3]; elems = B * A.twp; } // d(t) rows of the last backward pass (stride twp)
  else if (n == "d_dec_ah" && m->bf.on) { src = m->bf.trunk[1]; elems = B * A.dec_hidden; }   // d(hidden PReLU output) -> d(pre-activation), in place
  else if (n == "loc") { src = m->loc; elems = B * A.H * A.H * A.C; }
  else if (n == "scale") { src = m->scale; elems = B * A.H * A.H * A.C; }
  else if (n == "head_pre") {
    elems = B * A.dec_out * A.dec_out * 2 * A.C;
    if (nbytes != elems * sizeof(float)) {
      set_error("activation head_pre holds %zu bytes, caller passed %zu", elems * sizeof(float), nbytes);
      return DV_E_INVALID;
    }
    DV_HIP(hipSetDevice(m->ctx->device));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
    if (m->bf.on && m->bf.tpre_stale) {
      set_error("head_pre is not stored by a step that runs the head in the head conv's epilogue: keep the outputs "
                "(dv_model_set_keep_outputs) or set DV_BF_HEAD_FUSED=0");
      return DV_E_STATE;
    }
    if (m->bf.on) {
      // stamp-inner fp32 [Hd*Hd][NBp][16] -> [B][Hd][Hd][2C]
      const size_t Pn = (size_t)A.dec_out * A.dec_out, NBp = (size_t)m->bf.NBp, HC = (size_t)A.C2p;
      std::vector<float> tmp(Pn * NBp * HC);
      DV_HIP(hipMemcpy(tmp.data(), m->bf.tpre32, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t b = 0; b < B; ++b)
        for (size_t px = 0; px < Pn; ++px)
          memcpy(host + (b * Pn + px) * 2 * A.C, tmp.data() + (px * NBp + b) * HC, 2 * A.C * sizeof(float));
      return DV_OK;
    }
    DV_HIP(hipMemcpy2D(host, 2 * A.C * sizeof(float), m->tpre, A.C2p * sizeof(float), 2 * A.C * sizeof(float),
                       B * A.dec_out * A.dec_out, hipMemcpyDeviceToHost));
    return DV_OK;
  }
  else if (m->bf.on) {
    // stamp-inner bf16 [P][NBp][C] -> fp32 [B][P][C] on the host (tests only)
    const void* bsrc = nullptr;
    size_t Pn = 0, Cn = 0;
    if (n == "xn") { bsrc = m->bf.xh; Pn = (size_t)A.H * A.H; Cn = 16; }
    else if (n == "dec_in") { bsrc = m->bf.dec_in; Pn = (size_t)A.w0 * A.w0; Cn = A.cfg.filters[A.L - 1]; }
    else if (n == "d_dec_in") { bsrc = m->bf.d_dec_in; Pn = (size_t)A.w0 * A.w0; Cn = A.cfg.filters[A.L - 1]; }
    else if (n == "dec_ur") {
      // pre-activation of the decoder trunk's output: stamp-inner only when the trunk runs on the bf16 matrix cores
      // (btrunk.hip); "d_dec_in" is then d(that pre-activation), else the raw d(trunk output)
      if (!m->bf.trunk_mfma) {
        set_error("activation dec_ur: the dense trunk of this configuration runs on the fp32 kernels");
        return DV_E_STATE;
      }
      bsrc = m->bf.dec_ur; Pn = (size_t)A.w0 * A.w0; Cn = A.cfg.filters[A.L - 1];
    }
    else if (n == "d_head_pre") { bsrc = m->bf.dt; Pn = (size_t)A.dec_out * A.dec_out; Cn = (size_t)A.C2p; }
    else if (n.size() > 6 && (n.rfind("enc_du", 0) == 0 || n.rfind("dec_du", 0) == 0)) {
      // d(pre-activation) of conv layer j as the last backward pass left it (bf16; tests/test_gpu_bf16_layers.py)
      const int j = atoi(n.c_str() + 6);
      if (j < 0 || j >= 2 * A.L || (int)m->bf.du_enc.size() != 2 * A.L) return DV_E_INVALID;
      int hin, cin, hout, cout, s;
      if (n[0] == 'e') A.enc_layer(j, &hin, &cin, &hout, &cout, &s); else A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
      Pn = (size_t)hout * hout; Cn = cout;
      bsrc = n[0] == 'e' ? m->bf.du_enc[j] : m->bf.du_dec[j];
    }
    else if (n.size() > 5 && (n.rfind("enc_u", 0) == 0 || n.rfind("enc_a", 0) == 0 || n.rfind("dec_u", 0) == 0 || n.rfind("dec_a", 0) == 0)) {
      int j = atoi(n.c_str() + 5);
      if (j < 0 || j >= 2 * A.L) return DV_E_INVALID;
      int hin, cin, hout, cout, s;
      if (n[0] == 'e') A.enc_layer(j, &hin, &cin, &hout, &cout, &s); else A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
      Pn = (size_t)hout * hout; Cn = cout;
      bsrc = n[0] == 'e' ? (n[4] == 'u' ? m->bf.enc_u[j] : m->bf.enc_a[j]) : (n[4] == 'u' ? m->bf.dec_u[j] : m->bf.dec_a[j]);
    } else {
      set_error("activation '%s' is not exposed by the bf16 engine", name);
      return DV_E_INVALID;
    }
    elems = B * Pn * Cn;
    if (nbytes != elems * sizeof(float)) {
      set_error("activation %s holds %zu bytes, caller passed %zu", name, elems * sizeof(float), nbytes);
      return DV_E_INVALID;
    }
    if (!bsrc) {
      set_error("activation %s has not been computed yet", name);
      return DV_E_STATE;
    }
    const size_t NBp = (size_t)m->bf.NBp;
    std::vector<uint16_t> tmp(Pn * NBp * Cn);
    DV_HIP(hipSetDevice(m->ctx->device));
    DV_HIP(hipStreamSynchronize(m->ctx->stream));
    DV_HIP(hipMemcpy(tmp.data(), bsrc, tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b)
      for (size_t px = 0; px < Pn; ++px)
        for (size_t c = 0; c < Cn; ++c) {
          const uint32_t bits = (uint32_t)tmp[(px * NBp + b) * Cn + c] << 16;
          memcpy(host + (b * Pn + px) * Cn + c, &bits, 4);
        }
    return DV_OK;
  }
  else if (n == "xn") { src = m->xn; elems = B * A.H * A.H * A.C0p; }
  else if (n == "dec_in") { src = m->dec_ar; elems = B * A.w0 * A.w0 * A.cfg.filters[A.L - 1]; }
  else if (n == "dec_ur") { src = m->dec_ur; elems = B * A.w0 * A.w0 * A.cfg.filters[A.L - 1]; }   // its pre-activation (fp32 engine: rows)
  else if (n == "d_head_pre" || n == "enc_da0" || n.rfind("enc_du", 0) == 0 || n.rfind("dec_du", 0) == 0) {
    // gradients the last backward pass left in its per-step buffer pool (tests/test_gpu_layers.py)
    if (!m->du_valid) {
      set_error("activation %s: no backward pass with the per-step buffer pool has run (DV_NO_OVERLAP / profiling rotate three buffers)", name);
      return DV_E_STATE;
    }
    if (n == "d_head_pre") { src = m->gbufs[0]; elems = B * A.dec_out * A.dec_out * A.C2p; }
    else if (n == "enc_da0") { src = m->da_enc0; elems = B * A.H * A.H * A.cfg.filters[0]; }
    else {
      const int j = atoi(n.c_str() + 6);
      if (j < 0 || j >= 2 * A.L) return DV_E_INVALID;
      int hin, cin, hout, cout, s;
      if (n[0] == 'e') A.enc_layer(j, &hin, &cin, &hout, &cout, &s); else A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
      elems = B * hout * hout * cout;
      src = n[0] == 'e' ? m->du_enc[j] : m->du_dec[j];
    }
    if (!src) {
      set_error("activation %s is not materialised by this configuration", name);
      return DV_E_STATE;
    }
  }
  else if (n.rfind("enc_u", 0) == 0 || n.rfind("enc_a", 0) == 0 || n.rfind("dec_u", 0) == 0 || n.rfind("dec_a", 0) == 0) {
    int j = atoi(n.c_str() + 5);
    if (j < 0 || j >= 2 * A.L) return DV_E_INVALID;
    int hin, cin, hout, cout, s;
    if (n[0] == 'e') A.enc_layer(j, &hin, &cin, &hout, &cout, &s); else A.dec_layer(j, &hin, &cin, &hout, &cout, &s);
    elems = B * hout * hout * cout;
    src = n[0] == 'e' ? (n[4] == 'u' ? m->enc_u[j] : m->enc_a[j]) : (n[4] == 'u' ? m->dec_u[j] : m->dec_a[j]);
  } else {
    set_error("unknown activation '%s'", name);
    return DV_E_INVALID;
  }
  if (nbytes != elems * sizeof(float)) {
    set_error("activation %s holds %zu bytes, caller passed %zu", name, elems * sizeof(float), nbytes);
    return DV_E_INVALID;
  }
  DV_HIP(hipSetDevice(m->ctx->device));
  DV_HIP(hipStreamSynchronize(m->ctx->stream));
  DV_HIP(hipMemcpy(host, src, nbytes, hipMemcpyDeviceToHost));
  return DV_OK;
}

#ifdef DV_DEBUG_EXPORTS      // everything down to the matching #endif exists in libdebvader_hip_debug.so only
// ---- kernel micro-benchmarks (bench / tuning aid): time one layer-shaped launch on random data -----------
static int debug_buffers(dv_ctx* ctx, size_t nx, size_t nw, size_t ny, float** X, float** W, float** Y) {
  DV_HIP(hipSetDevice(ctx->device));
  DV_HIP(hipMalloc((void**)X, nx * sizeof(float)));
  DV_HIP(hipMalloc((void**)W, nw * sizeof(float)));
  DV_HIP(hipMalloc((void**)Y, ny * sizeof(float)));
  std::vector<float> h(std::max(nx, nw));
  uint32_t st = 12345u;
  for (auto& v : h) {
    st = st * 1664525u + 1013904223u;
    v = ((st >> 8) * (1.0f / 8388608.0f)) - 1.0f;
  }
  DV_HIP(hipMemcpy(*X, h.data(), nx * sizeof(float), hipMemcpyHostToDevice));
  DV_HIP(hipMemcpy(*W, h.data(), nw * sizeof(float), hipMemcpyHostToDevice));
  DV_HIP(hipMemset(*Y, 0, ny * sizeof(float)));
  DV_HIP(hipDeviceSynchronize());     // hipMemset runs on the null stream, the kernels under test on a non-blocking one
  return OK;
}

int dv_debug_gconv(dv_ctx* ctx, int32_t NB, int32_t Hs, int32_t Cs, int32_t Ht, int32_t Ct, int32_t stride,
                   int32_t pb, int32_t dgrad_form, int32_t nmajor, int32_t epi, int32_t single_tap, int32_t tile,
                   int32_t iters, float* ms_out) {
  if (!ctx || !ms_out || iters < 1) return DV_E_INVALID;
  dv_model m;
  m.ctx = ctx;
  float *X, *W, *Y;
  size_t nx = (size_t)NB * Hs * Hs * Cs, nw = (size_t)9 * Cs * Ct + 4096, ny = (size_t)NB * Ht * Ht * Ct;
  DV_TRY(debug_buffers(ctx, nx, nw + ny / NB, ny, &X, &W, &Y));
  float* bias = W + 9 * (size_t)Cs * Ct;     // reuse the tail as bias / alpha
  float* Y2 = nullptr;
  DV_HIP(hipMalloc((void**)&Y2, ny * sizeof(float)));
  m.ws1_elems = (size_t)16 << 20;
  DV_HIP(hipMalloc((void**)&m.ws1, m.ws1_elems * sizeof(float)));
  DV_HIP(hipMalloc((void**)&m.zero_page, 256));
  DV_HIP(hipMemsetAsync(m.zero_page, 0, 256, ctx->stream));
  const bool timeline = tile >= 7000;
  if (timeline) {
    tile -= 7000;
    if (tile == 99) tile = -1;
    DV_HIP(hipMemsetAsync(m.ws1 + m.ws1_elems - (1 << 16), 0, (1 << 16) * sizeof(float), ctx->stream));
    debug_set_gconv2_dbg(2, m.ws1 + m.ws1_elems - (1 << 16));
    debug_set_gconv_s2_dbg(reinterpret_cast<unsigned*>(m.ws1 + m.ws1_elems - (1 << 16)));
  }
  if (tile >= 4000) {
    debug_set_gconv2_prio(4);   // 4: loads in front of the MFMA block (pre-interleave order)
    tile -= 4000;
    if (tile == 99) tile = -1;
  }
  const bool stamps = tile >= 500 && tile < 1000;
  if (stamps) {
    tile -= 500;
    if (tile == 99) tile = -1;
    debug_set_gconv2_dbg(1, m.ws1 + m.ws1_elems - 64);
  }
  g_force_v1 = tile >= 1000;
  if (g_force_v1) debug_set_gconv_tile(tile - 1000 == 99 ? -1 : tile - 1000); else debug_set_gconv2_tile(tile);
  hipEvent_t a, b;
  DV_HIP(hipEventCreate(&a));
  DV_HIP(hipEventCreate(&b));
  int st = OK;
  for (int it = -2; it < iters && st == OK; ++it) {
    if (it == 0) DV_HIP(hipEventRecord(a, ctx->stream));
    if (dgrad_form)
      st = gconv_dgrad(&m, X, W, nmajor != 0, bias, bias, Y, Y2, epi, NB, Hs, Cs, Ht, Ct, stride, pb);
    else
      st = gconv_fprop(&m, X, W, nmajor != 0, bias, bias, Y, Y2, epi, NB, Hs, Cs, Ht, Ct, stride, pb,
                       single_tap != 0);
  }
  DV_HIP(hipEventRecord(b, ctx->stream));
  DV_HIP(hipEventSynchronize(b));
  debug_set_gconv_tile(-1);
  debug_set_gconv2_tile(-1);
  debug_set_gconv2_dbg(0, nullptr);
  debug_set_gconv_s2_dbg(nullptr);
  debug_set_gconv2_prio(0);
  g_force_v1 = false;
  if (timeline) {
    // per-workgroup timeline of the LAST launch (s_memrealtime ticks of 10 ns): start, loop start, loop end, end
    std::vector<unsigned> h(1 << 16);
    DV_HIP(hipMemcpy(h.data(), m.ws1 + m.ws1_elems - (1 << 16), h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    unsigned t0 = 0xffffffffu, t3 = 0;
    int n = 0;
    for (int i = 0; i < (1 << 14); ++i)
      if (h[4 * i + 3]) { t0 = std::min(t0, h[4 * i]); t3 = std::max(t3, h[4 * i + 3]); ++n; }
    double sp = 0, sl = 0, se = 0, last_start = 0, first_end = 1e9;
    for (int i = 0; i < (1 << 14); ++i)
      if (h[4 * i + 3]) {
        sp += h[4 * i + 1] - h[4 * i]; sl += h[4 * i + 2] - h[4 * i + 1]; se += h[4 * i + 3] - h[4 * i + 2];
        last_start = std::max(last_start, (double)(h[4 * i] - t0)); first_end = std::min(first_end, (double)(h[4 * i + 3] - t0));
      }
    {
      double a = 0, b = 0, c = 0, dd = 0;
      int k = 0;
      for (int i = 0; i < (1 << 13); ++i)
        if (h[4 * i + 3] && h[(1 << 15) + 4 * i]) {
          a += h[(1 << 15) + 4 * i] - h[4 * i]; b += h[(1 << 15) + 4 * i + 1] - h[(1 << 15) + 4 * i];
          c += h[(1 << 15) + 4 * i + 2] - h[(1 << 15) + 4 * i + 1]; dd += h[4 * i + 1] - h[(1 << 15) + 4 * i + 2]; ++k;
        }
      if (k) fprintf(stderr, "  prologue split: row table + barrier %.2f us, address setup + first load issue %.2f us, load latency %.2f us, LDS store + second load + barrier %.2f us\n",
                     a / k * 0.01, b / k * 0.01, c / k * 0.01, dd / k * 0.01);
    }
    fprintf(stderr, "  timeline: %d workgroups, span %.1f us; mean prologue %.2f us, loop %.2f us, epilogue %.2f us; last start at %.1f us, first end at %.1f us\n",
            n, (t3 - t0) * 0.01, sp / n * 0.01, sl / n * 0.01, se / n * 0.01, last_start * 0.01, first_end * 0.01);
    for (int i = 0; i < n && i < 1 << 14; i += std::max(1, n / 16))
      fprintf(stderr, "    wg %5d: start %.1f loop %.1f-%.1f end %.1f us\n", i, (h[4 * i] - t0) * 0.01, (h[4 * i + 1] - t0) * 0.01, (h[4 * i + 2] - t0) * 0.01, (h[4 * i + 3] - t0) * 0.01);
  }
  if (stamps) {
    float h[32];
    DV_HIP(hipMemcpy(h, m.ws1 + m.ws1_elems - 64, sizeof h, hipMemcpyDeviceToHost));
    for (int w = 0; w < 4; ++w)
      fprintf(stderr, "  wave %d: load-issue %.0f  compute %.0f  wait+store %.0f  barrier %.0f cycles over %.0f chunks; clock %.0f MHz\n", w, h[8 * w], h[8 * w + 1], h[8 * w + 2], h[8 * w + 3], h[8 * w + 4], h[8 * w + 6] > 0 ? h[8 * w + 5] / h[8 * w + 6] * 100.f : 0.f);
  }
  float ms = 0;
  DV_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = ms / iters;
  (void)hipFree(X); (void)hipFree(W); (void)hipFree(Y); (void)hipFree(Y2); (void)hipFree(m.ws1); (void)hipFree(m.zero_page);
  for (void* q : m.allocs) (void)hipFree(q);      // Winograd weights registered on the fly
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return st;
}

static int debug_gather_check(dv_ctx* ctx, int32_t NB, int32_t Hs, int32_t Cs, int32_t Ht, int32_t Ct, int32_t stride,
                              int32_t pb, int32_t dgrad_form, int32_t nmajor, int32_t epi, int32_t tile, float* out3);

// Cross-check of the specialised gather-GEMM kernels (gconv_strip, gconv_s2) against the general gconv2 path on the
// same pseudo-random operands: out2 = {max |difference| over both outputs, max |reference|}.
// epi bit 8 selects the gather cross-check instead (debug_gather_check below): epilogue in bits 0-7, tile code + 1 in bits
// 16-23 (0 = automatic), THREE floats out.
int dv_debug_gconv_check(dv_ctx* ctx, int32_t NB, int32_t Hs, int32_t Cs, int32_t Ht, int32_t Ct, int32_t stride,
                         int32_t pb, int32_t dgrad_form, int32_t nmajor, int32_t epi, float* out2) {
  if (!ctx || !out2) return DV_E_INVALID;
  if (epi & 0x100)
    return debug_gather_check(ctx, NB, Hs, Cs, Ht, Ct, stride, pb, dgrad_form, nmajor, epi & 0xff, ((epi >> 16) & 0xff) - 1, out2);
  dv_model m;
  m.ctx = ctx;
  float *X, *W, *Y;
  const size_t nx = (size_t)NB * Hs * Hs * Cs, nw = (size_t)9 * Cs * Ct + 4096, ny = (size_t)NB * Ht * Ht * Ct;
  const size_t nal = (size_t)Ht * Ht * Ct;
  DV_TRY(debug_buffers(ctx, nx, nw + nal, ny, &X, &W, &Y));
  float* bias = W + 9 * (size_t)Cs * Ct;
  float* alpha = bias + 4096;
  float* bufs[3] = {nullptr, nullptr, nullptr};                  // A of the fast path, U and A of the reference
  for (auto& b : bufs) DV_HIP(hipMalloc((void**)&b, ny * sizeof(float)));
  m.ws1_elems = (size_t)1 << 20;
  DV_HIP(hipMalloc((void**)&m.ws1, m.ws1_elems * sizeof(float)));
  DV_HIP(hipMalloc((void**)&m.zero_page, 256));
  DV_HIP(hipMemsetAsync(m.zero_page, 0, 256, ctx->stream));
  int st = OK;
  for (int pass = 0; pass < 2 && st == OK; ++pass) {
    g_no_special = pass == 1;
    float* U = pass == 0 ? Y : bufs[1];
    float* A = pass == 0 ? bufs[0] : bufs[2];
    DV_HIP(hipMemsetAsync(U, 0, ny * sizeof(float), ctx->stream));
    DV_HIP(hipMemsetAsync(A, 0, ny * sizeof(float), ctx->stream));
    if (dgrad_form)
      st = gconv_dgrad(&m, X, W, nmajor != 0, bias, alpha, U, A, epi, NB, Hs, Cs, Ht, Ct, stride, pb);
    else
      st = gconv_fprop(&m, X, W, nmajor != 0, bias, alpha, U, A, epi, NB, Hs, Cs, Ht, Ct, stride, pb, false);
  }
  g_no_special = false;
  DV_HIP(hipStreamSynchronize(ctx->stream));
  if (st == OK) {
    std::vector<float> a(ny), b(ny);
    double md = 0, mr = 0;
    for (int k = 0; k < 2; ++k) {
      DV_HIP(hipMemcpy(a.data(), k == 0 ? Y : bufs[0], ny * sizeof(float), hipMemcpyDeviceToHost));
      DV_HIP(hipMemcpy(b.data(), k == 0 ? bufs[1] : bufs[2], ny * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < ny; ++i) {
        md = std::max(md, (double)fabsf(a[i] - b[i]));
        mr = std::max(mr, (double)fabsf(b[i]));
      }
    }
    out2[0] = (float)md;
    out2[1] = (float)mr;
  }
  (void)hipFree(X); (void)hipFree(W); (void)hipFree(Y); (void)hipFree(m.ws1); (void)hipFree(m.zero_page);
  for (auto& b : bufs) (void)hipFree(b);
  for (void* q : m.allocs) (void)hipFree(q);      // Winograd weights registered on the fly
  return st;
}

// The gather-GEMM kernels (gconv2, gconv_s2) on the select form of their gathers and on the range-checked buffer loads, same
// launch, same pseudo-random operands.  X and W each lie INSIDE a larger allocation between two bands of NaN (64 KiB each):
// the descriptors cover the tensors alone, so a buffer load that strays past a tensor shows as a NaN or a differing word,
// never as a fault.  out3 = {output words (U and A) whose bit patterns differ, NaNs in the buffer path's outputs,
// max |select-path output|}.  tile: -1 automatic, else the tile code of both kernel families.
static int debug_gather_check(dv_ctx* ctx, int32_t NB, int32_t Hs, int32_t Cs, int32_t Ht, int32_t Ct, int32_t stride,
                              int32_t pb, int32_t dgrad_form, int32_t nmajor, int32_t epi, int32_t tile, float* out3) {
  if (!ctx || !out3 || NB < 1 || Hs < 1 || Ht < 1 || Cs < 1 || Ct < 1) return DV_E_INVALID;
  dv_model m;
  m.ctx = ctx;
  DV_HIP(hipSetDevice(ctx->device));
  const bool single_tap = !dgrad_form && Hs == 1 && Ht == 1 && stride == 1;
  const size_t band = 16384;                                     // floats: 64 KiB in front of and behind each tensor
  const size_t nx = (size_t)NB * Hs * Hs * Cs, nw = (size_t)(single_tap ? 1 : 9) * Cs * Ct, ny = (size_t)NB * Ht * Ht * Ct;
  const size_t nal = (size_t)Ht * Ht * Ct, npar = (size_t)Ct + nal;
  DevBuf<float> Xa, Wa, Par, out[4];                             // U, A of the select path; U, A of the buffer path
  DV_TRY(Xa.alloc(nx + 2 * band));
  DV_TRY(Wa.alloc(nw + 2 * band));
  DV_TRY(Par.alloc(npar));
  for (auto& b : out) DV_TRY(b.alloc(ny));
  {
    std::vector<float> h(std::max(std::max(nx, nw) + 2 * band, npar));
    uint32_t st = 12345u;
    auto fill = [&](size_t n0, size_t n) {           // n0 NaNs, n values in [-1, 1), n0 NaNs
      for (size_t i = 0; i < n0 + n + n0; ++i) {
        st = st * 1664525u + 1013904223u;
        h[i] = (i < n0 || i >= n0 + n) ? __builtin_nanf("") : ((st >> 8) * (1.0f / 8388608.0f)) - 1.0f;
      }
    };
    fill(band, nx);
    DV_HIP(hipMemcpy(Xa.get(), h.data(), (nx + 2 * band) * sizeof(float), hipMemcpyHostToDevice));
    fill(band, nw);
    DV_HIP(hipMemcpy(Wa.get(), h.data(), (nw + 2 * band) * sizeof(float), hipMemcpyHostToDevice));
    fill(0, npar);
    DV_HIP(hipMemcpy(Par.get(), h.data(), npar * sizeof(float), hipMemcpyHostToDevice));
  }
  const float* X = Xa.get() + band;
  const float* W = Wa.get() + band;
  const float* bias = Par.get();
  const float* alpha = Par.get() + Ct;
  DevBuf<float> ws1, zero_page;
  m.ws1_elems = (size_t)1 << 20;
  DV_TRY(ws1.alloc(m.ws1_elems));
  DV_TRY(zero_page.alloc(64));
  m.ws1 = ws1.get();
  m.zero_page = zero_page.get();
  DV_HIP(hipMemset(m.zero_page, 0, 256));
  for (auto& b : out) DV_HIP(hipMemset(b.get(), 0, ny * sizeof(float)));
  DV_HIP(hipDeviceSynchronize());     // hipMemset runs on the null stream, the kernels under test on a non-blocking one
  const bool was_on = buffer_gather_on();
  if (tile >= 0) {
    debug_set_gconv2_tile(tile);
    debug_set_gconv_s2_tile(tile);
  }
  int st = OK;
  for (int pass = 0; pass < 2 && st == OK; ++pass) {
    debug_set_buffer_gather(pass);
    float* U = out[2 * pass].get();
    float* A = out[2 * pass + 1].get();
    if (dgrad_form)
      st = gconv_dgrad(&m, X, W, nmajor != 0, bias, alpha, U, A, epi, NB, Hs, Cs, Ht, Ct, stride, pb);
    else
      st = gconv_fprop(&m, X, W, nmajor != 0, bias, alpha, U, A, epi, NB, Hs, Cs, Ht, Ct, stride, pb, single_tap);
  }
  debug_set_buffer_gather(was_on ? 1 : 0);
  debug_set_gconv2_tile(-1);
  debug_set_gconv_s2_tile(-1);
  const hipError_t se = hipStreamSynchronize(ctx->stream);
  if (st == OK && se != hipSuccess) st = hip_fail(se, "hipStreamSynchronize", __FILE__, __LINE__);
  if (st == OK) {
    std::vector<uint32_t> a(ny), b(ny);
    double ndiff = 0, nnan = 0, mr = 0;
    for (int k = 0; k < 2 && st == OK; ++k) {
      const hipError_t e1 = hipMemcpy(a.data(), out[k].get(), ny * sizeof(float), hipMemcpyDeviceToHost);
      const hipError_t e2 = hipMemcpy(b.data(), out[2 + k].get(), ny * sizeof(float), hipMemcpyDeviceToHost);
      if (e1 != hipSuccess || e2 != hipSuccess) {
        st = hip_fail(e1 != hipSuccess ? e1 : e2, "hipMemcpy", __FILE__, __LINE__);
        break;
      }
      for (size_t i = 0; i < ny; ++i) {
        float fa, fb;
        memcpy(&fa, &a[i], 4);
        memcpy(&fb, &b[i], 4);
        if (a[i] != b[i]) ndiff += 1;
        if (fb != fb) nnan += 1;
        if (fa == fa) mr = std::max(mr, (double)fabsf(fa));
      }
    }
    out3[0] = (float)ndiff;
    out3[1] = (float)nnan;
    out3[2] = (float)mr;
  }
  for (void* q : m.allocs) (void)hipFree(q);      // Winograd weights registered on the fly
  return st;
}

// Winograd-domain weight gradient (wino.hip) against the direct kernels on the same pseudo-random operands:
// out2 = {max |difference|, max |reference|}
int dv_debug_wgrad_check(dv_ctx* ctx, int32_t NB, int32_t H, int32_t Cx, int32_t Cy, float* out2) {
  if (!ctx || !out2) return DV_E_INVALID;
  dv_model m;
  m.ctx = ctx;
  float *X, *Yb, *out;
  const size_t nx = (size_t)NB * H * H * Cx, ny = (size_t)NB * H * H * Cy, nw = (size_t)9 * Cx * Cy;
  DV_TRY(debug_buffers(ctx, nx, ny, 2 * nw, &X, &Yb, &out));
  m.ws1_elems = (size_t)16 << 20;
  DV_HIP(hipMalloc((void**)&m.ws1, m.ws1_elems * sizeof(float)));
  DV_HIP(hipMalloc((void**)&m.zero_page, 256));
  DV_HIP(hipMemset(m.zero_page, 0, 256));
  DV_HIP(hipDeviceSynchronize());   // (hipMemset runs on the null stream; the kernels on a non-blocking one)
  int st = OK;
  for (int pass = 0; pass < 2 && st == OK; ++pass) {
    g_no_wino = pass == 1;
    m.wino_wcount = 0;
    st = wgrad(&m, X, H, Cx, Yb, H, Cy, NB, 1, 1, false, out + pass * nw, Cx, Cx, nullptr);
  }
  g_no_wino = false;
  DV_HIP(hipStreamSynchronize(ctx->stream));
  if (st == OK) {
    std::vector<float> a(nw), b(nw);
    DV_HIP(hipMemcpy(a.data(), out, nw * sizeof(float), hipMemcpyDeviceToHost));
    DV_HIP(hipMemcpy(b.data(), out + nw, nw * sizeof(float), hipMemcpyDeviceToHost));
    double md = 0, mr = 0;
    for (size_t i = 0; i < nw; ++i) {
      md = std::max(md, (double)fabsf(a[i] - b[i]));
      mr = std::max(mr, (double)fabsf(b[i]));
    }
    out2[0] = (float)md;
    out2[1] = (float)mr;
  }
  (void)hipFree(X); (void)hipFree(Yb); (void)hipFree(out); (void)hipFree(m.ws1); (void)hipFree(m.zero_page);
  for (void* q : m.allocs) (void)hipFree(q);
  return st;
}

int dv_debug_winograd(int32_t on) {
  g_no_wino = on == 0;
  if (on >= 1) debug_set_wino_variant(on == 3 ? 1 : 2);       // 3: the first-generation eight-wave kernel
  return DV_OK;
}

int dv_debug_fuse_prelu_bwd(int32_t on) {
  g_fuse_prelu_bwd = on != 0;
  return DV_OK;
}

int dv_debug_general_kernels(int32_t on) {
  g_no_special = (on & 1) != 0;
  debug_set_buffer_gather((on & 2) == 0);        // bit 1: select form of the gconv2 / gconv_s2 gathers
  return DV_OK;
}

int dv_debug_mfma_peak(dv_ctx* ctx, int32_t blocks, int32_t iters, int32_t nacc, int32_t randomize, float* out3) {
  if (!ctx || !out3) return DV_E_INVALID;
  DV_HIP(hipSetDevice(ctx->device));
  float* out;
  DV_HIP(hipMalloc((void**)&out, ((size_t)blocks * 256 + 16) * sizeof(float)));
  hipEvent_t a, b;
  DV_HIP(hipEventCreate(&a));
  DV_HIP(hipEventCreate(&b));
  if (nacc != 36) nacc = 16;
  DV_TRY(debug_mfma_peak(out, blocks, iters, nacc, randomize, ctx->stream));
  DV_HIP(hipEventRecord(a, ctx->stream));
  DV_TRY(debug_mfma_peak(out, blocks, iters, nacc, randomize, ctx->stream));
  DV_HIP(hipEventRecord(b, ctx->stream));
  DV_HIP(hipEventSynchronize(b));
  float ms = 0;
  DV_HIP(hipEventElapsedTime(&ms, a, b));
  float h[2];
  DV_HIP(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
  out3[0] = (float)((double)blocks * 4 * iters * nacc * 2048.0 / (ms * 1e-3) / 1e12);   // TFLOP/s
  out3[1] = h[1] > 0 ? h[0] / h[1] * 100.0f : 0.f;                                       // in-kernel clock, MHz
  out3[2] = h[0] / ((float)iters * nacc);                                                // cycles per MFMA
  (void)hipFree(out);
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return DV_OK;
}

int dv_debug_wgrad(dv_ctx* ctx, int32_t NB, int32_t Hx, int32_t Cx, int32_t Hy, int32_t Cy, int32_t sx, int32_t pb,
                   int32_t single_tap, int32_t iters, float* ms_out) {
  if (!ctx || !ms_out || iters < 1) return DV_E_INVALID;
  dv_model m;
  m.ctx = ctx;
  float *X, *Yb, *out;
  size_t nx = (size_t)NB * Hx * Hx * Cx, ny = (size_t)NB * Hy * Hy * Cy, nw = (size_t)9 * Cx * Cy;
  DV_TRY(debug_buffers(ctx, nx, ny, nw, &X, &Yb, &out));
  m.ws1_elems = (size_t)16 << 20;
  DV_HIP(hipMalloc((void**)&m.ws1, m.ws1_elems * sizeof(float)));
  DV_HIP(hipMalloc((void**)&m.zero_page, 256));
  DV_HIP(hipMemset(m.zero_page, 0, 256));
  DV_HIP(hipDeviceSynchronize());   // (hipMemset runs on the null stream; the kernels on a non-blocking one)
  hipEvent_t a, b;
  DV_HIP(hipEventCreate(&a));
  DV_HIP(hipEventCreate(&b));
  int st = OK;
  // bit 8: the fused first-layer form (PReLU backward inside the kernel); Yb then plays d(activation)
  const bool fused = (single_tap & 0x100) != 0 && Cx == 8;
  single_tap &= 0xff;
  float *U = nullptr, *al = nullptr, *gout = nullptr;
  FuseBwd fz{nullptr, 0, 0, true};
  if (fused) {
    const size_t E = (size_t)Hy * Hy * Cy;
    DV_HIP(hipMalloc((void**)&U, ny * sizeof(float)));
    DV_HIP(hipMemcpy(U, Yb, ny * sizeof(float), hipMemcpyDeviceToDevice));
    DV_HIP(hipMalloc((void**)&al, E * sizeof(float)));
    DV_HIP(hipMemset(al, 0, E * sizeof(float)));
    DV_HIP(hipDeviceSynchronize());
    DV_HIP(hipMalloc((void**)&gout, (E + 64) * sizeof(float)));
    m.ws2_elems = 32 * E;
    DV_HIP(hipMalloc((void**)&m.ws2, m.ws2_elems * sizeof(float)));
    m.ws3_elems = (size_t)1024 * Cy;
    DV_HIP(hipMalloc((void**)&m.ws3, m.ws3_elems * sizeof(float)));
    fz.u = U;
    fz.alpha_ptr = al;
    fz.dalpha_out = gout;
    fz.dbias_out = gout + E;
  }
  DV_HIP(hipEventRecord(a, ctx->stream));
  for (int it = -2; it < iters && st == OK; ++it) {
    if (it == 0) DV_HIP(hipEventRecord(a, ctx->stream));
    g_force_v1 = (single_tap & 2) != 0;
    debug_set_strip(single_tap >> 2);
    m.wino_wcount = 0;
    st = wgrad(&m, X, Hx, Cx, Yb, Hy, Cy, NB, sx, pb, (single_tap & 1) != 0, out, Cx, Cx, fused ? &fz : nullptr);
    g_force_v1 = false;
    debug_set_strip(0);
  }
  DV_HIP(hipEventRecord(b, ctx->stream));
  DV_HIP(hipEventSynchronize(b));
  float ms = 0;
  DV_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = ms / iters;
  if ((single_tap >> 2) == 4) {
    float h[16];
    DV_HIP(hipMemcpy(h, m.ws1 + m.ws1_elems - 64, sizeof h, hipMemcpyDeviceToHost));
    for (int w = 0; w < 4; ++w)
      fprintf(stderr, "  wave %d: barrier %.0f  dma-issue %.0f  compute %.0f cycles over %.0f strips\n", w, h[4 * w], h[4 * w + 1], h[4 * w + 2], h[4 * w + 3]);
  }
  (void)hipFree(X); (void)hipFree(Yb); (void)hipFree(out); (void)hipFree(m.ws1); (void)hipFree(m.zero_page);
  for (void* q : m.allocs) (void)hipFree(q);      // Winograd slabs allocated on the fly
  if (fused) {
    (void)hipFree(U); (void)hipFree(al); (void)hipFree(gout); (void)hipFree(m.ws2); (void)hipFree(m.ws3);
    m.ws2 = m.ws3 = nullptr;
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return st;
}

#endif   // DV_DEBUG_EXPORTS

int dv_ctx_comm_info(dv_ctx* c, int32_t* comm_ranks, int32_t* comm_rank, int32_t* device, char* bus_id, size_t bus_len,
                     int32_t* rehearsal) {
  if (!c) return DV_E_INVALID;
  int n = 0, r = 0;
  if (c->comm) {
    DV_NCCL(ncclCommCount(c->comm, &n));
    DV_NCCL(ncclCommUserRank(c->comm, &r));
  }
  if (comm_ranks) *comm_ranks = n;
  if (comm_rank) *comm_rank = r;
  if (device) *device = c->device;
  if (bus_id && bus_len) {
    bus_id[0] = 0;
    if (bus_len >= 16) (void)hipDeviceGetPCIBusId(bus_id, (int)bus_len, c->device);
  }
  if (rehearsal) *rehearsal = c->fake_peers ? 1 : 0;
  return DV_OK;
}

static void cprof_drain(dv_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, int64_t* n, double* ms) {
  for (auto& pr : v) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) {
      *ms += t;
      *n += 1;
    }
    c->cprof_pool.push_back(pr.first);
    c->cprof_pool.push_back(pr.second);
  }
  v.clear();
}

int dv_comm_prof_enable(dv_ctx* c, int32_t on) {
  if (!c) return DV_E_INVALID;
  c->cprof_on = on != 0;
  return DV_OK;
}

int dv_comm_prof_read(dv_ctx* c, int64_t* n_collectives, double* comm_ms, int64_t* n_waits, double* exposed_ms) {
  if (!c) return DV_E_INVALID;
  DV_HIP(hipSetDevice(c->device));
  DV_HIP(hipStreamSynchronize(c->stream));
  if (c->comm_stream) DV_HIP(hipStreamSynchronize(c->comm_stream));
  int64_t n1 = 0, n2 = 0;
  double a = 0, b = 0;
  cprof_drain(c, c->cprof_comm, &n1, &a);
  cprof_drain(c, c->cprof_wait, &n2, &b);
  if (n_collectives) *n_collectives = n1;
  if (comm_ms) *comm_ms = a;
  if (n_waits) *n_waits = n2;
  if (exposed_ms) *exposed_ms = b;
  return DV_OK;
}

int dv_prof_enable(dv_model* m, int32_t on) {
  if (!m) return DV_E_INVALID;
  DV_TRY(prof_flush(m));
  m->prof_on = on != 0;
  return DV_OK;
}
int dv_prof_read(dv_model* m, int32_t klass, int64_t* launches, double* total_ms) {
  if (!m || klass < 0 || klass > 2) return DV_E_INVALID;
  DV_TRY(prof_flush(m));
  if (launches) *launches = m->prof_n[klass];
  if (total_ms) *total_ms = m->prof_ms[klass];
  return DV_OK;
}
int dv_prof_read_family(dv_model* m, int32_t fam, char* name, size_t name_len, int64_t* launches, double* total_ms,
                        double* flops, double* executed_flops, double* algorithmic_bytes) {
  if (!m) return DV_E_INVALID;
  if (fam < 0 || fam >= PF_COUNT) return DV_E_INVALID;
  DV_TRY(prof_flush(m));
  if (name && name_len) snprintf(name, name_len, "%s", kProfFamName[fam]);
  if (launches) *launches = m->fam_launches[fam];
  if (total_ms) *total_ms = m->fam_ms[fam];
  if (flops) *flops = m->fam_flops[fam];
  if (executed_flops) *executed_flops = m->fam_exec[fam];
  if (algorithmic_bytes) *algorithmic_bytes = m->fam_bytes[fam];
  return DV_OK;
}

int dv_prof_reset(dv_model* m) {
  if (!m) return DV_E_INVALID;
  DV_TRY(prof_flush(m));
  for (int k = 0; k < 3; ++k) {
    m->prof_n[k] = 0;
    m->prof_ms[k] = 0;
  }
  for (int f = 0; f < PF_COUNT; ++f) {
    m->fam_launches[f] = 0;
    m->fam_ms[f] = 0;
    m->fam_flops[f] = 0;
    m->fam_exec[f] = 0;
    m->fam_bytes[f] = 0;
  }
  return DV_OK;
}

}  // extern "C"
