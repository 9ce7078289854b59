// Shared declarations for the debvader_amd HIP engine (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <memory>
#include <utility>
#include <vector>

struct dv_detect_params;   // include/debvader_hip.h: the detector reads the C ABI's parameter block as it is (DetectRequest)

namespace dv {

// status codes (mirrored in include/debvader_hip.h)
enum : int {
  OK = 0,
  E_INVALID = -1,
  E_HIP = -2,
  E_NOMEM = -3,
  E_RCCL = -4,
  E_STATE = -5,
  E_NODEVICE = -6,
};

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define DV_HIP(call)                                                     \
  do {                                                                   \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return dv::hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)

#define DV_TRY(call)            \
  do {                          \
    int s__ = (call);           \
    if (s__ != dv::OK) return s__; \
  } while (0)

// ---- owning buffers of the host code --------------------------------------------------------------------------------
// DevBuf<T>: elements of device memory that the destructor frees; PinBuf<T>: the same of pinned host memory.  Move-only, no
// pool, no sharing.  alloc() gets at least one element and reports a failure through hip_fail with the caller's file and
// line; ensure() only ever grows (the old content is dropped).
template <typename T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }   // (o frees the old one)
  ~DevBuf() { reset(); }
  int alloc(size_t count, const char* what = Pinned ? "hipHostMalloc" : "hipMalloc", const char* file = __builtin_FILE(),
            int line = __builtin_LINE()) {
    reset();
    cap_ = count ? count : 1;
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, cap_ * sizeof(T), hipHostMallocDefault)
                                : hipMalloc((void**)&p_, cap_ * sizeof(T));
    if (e == hipSuccess) return OK;
    p_ = nullptr; cap_ = 0;
    return hip_fail(e, what, file, line);
  }
  int ensure(size_t count, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    return count <= cap_ ? OK : alloc(count, Pinned ? "hipHostMalloc" : "hipMalloc", file, line);
  }
  void reset() {
    if (p_) Pinned ? (void)hipHostFree(p_) : (void)hipFree(p_);
    p_ = nullptr; cap_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
 private:
  T* p_ = nullptr;
  size_t cap_ = 0;     // elements
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// A failed call must not free buffers that queued work may still read: declared AFTER the buffers it protects (so that it
// runs first), it waits for the given streams when the scope is left - unless the call succeeded and dismissed it.
struct StreamDrain {
  hipStream_t streams[3];
  bool armed = true;
  explicit StreamDrain(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr) : streams{a, b, c} {}
  StreamDrain(const StreamDrain&) = delete;
  ~StreamDrain() {
    for (hipStream_t q : streams)
      if (armed && q) (void)hipStreamSynchronize(q);
  }
  void dismiss() { armed = false; }
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// MEASUREMENT switches (DV_EXP_*, DV_TIME_ENQUEUE) leave work out of a step to price it: they give WRONG results, so they
// exist only in the development library (libdebvader_hip_debug.so, -DDV_DEBUG_EXPORTS), which announces every one that is
// set on stderr.  In the product library DV_EXP_SWITCH(...) is the constant 0: the environment is not read, the names do
// not appear in the binary (tests/test_abi_and_host.py checks `strings`), and the branches fold away.
#ifdef DV_DEBUG_EXPORTS
int exp_switch(const char* name);        // engine.hip: atoi of the variable (unset or "0": off), one warning per name
#define DV_EXP_SWITCH(name) ::dv::exp_switch(name)
#else
#define DV_EXP_SWITCH(name) 0
#endif

#ifdef __HIPCC__
// Range-checked gathers (gconv2.hip, gconv_s2.hip).  One raw-buffer descriptor per gathered tensor whose record count is
// the tensor's byte size: a buffer load whose byte offset lies outside [0, bytes) returns zeros, so a lane that has to
// contribute zeros only needs an out-of-range offset (the byte size itself) and nothing after the load.  The descriptor
// is built from kernel arguments passed through readfirstlane, once per kernel: the compiler then keeps it in scalar
// registers and every load is a single buffer_load_dwordx4 ... offen.  Everything that decides validity is in the
// per-lane offset; the scalar offset operand stays 0.
typedef __amdgpu_buffer_rsrc_t BufRsrc;
__device__ __forceinline__ BufRsrc make_gather_rsrc(const float* base, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  void* q = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ f32x4 gather_b128(BufRsrc rs, unsigned byte_off) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 0);
  return __builtin_bit_cast(f32x4, v);
}
// Bytes of headroom the out-of-range offsets need above a tensor of `bytes` bytes: an invalid lane's offset is `bytes`
// plus a wave-uniform term below `uniform_max` bytes, and the access adds 16.  False: take the select form.
inline bool gather_range_fits(unsigned long long bytes, unsigned long long uniform_max) {
  return bytes + uniform_max + 16ull <= 0xffffffffull;
}

// Philox4x32-10 and the standard normal the engine derives from it (pairs (0,1), (2,3) of a block are one
// Box-Muller draw): shared by the sampler and the sampled-"mse" metric of the head kernels
__device__ __forceinline__ void dv_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float dv_philox_normal(unsigned row, unsigned col, unsigned stream, unsigned long long seed) {
  unsigned r[4];
  dv_philox4x32_10(row, col >> 2, stream, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
  const int a = col & 3;
  const float u1 = ((float)r[a & ~1] + 1.0f) * 2.3283064365386963e-10f;
  const float u2 = ((float)r[(a & ~1) + 1] + 1.0f) * 2.3283064365386963e-10f;
  const float rad = sqrtf(-2.0f * logf(fminf(u1, 1.0f)));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  return (a & 1) ? rad * sn : rad * cs;
}
#endif

// ---------------------------------------------------------------------------------------------
// Gather-GEMM ("gconv"): Y[m, n] = sum_k A[m, k] * B[k, n]  with
//   m  -> (stamp nb, class-grid row i, class-grid col j),   M = NB*Hc*Wc
//   k  -> (tap t, input channel c),                        K = ntaps*Cin
//   A[m,k] = X[nb, i*sin + dh[t], j*sin + dw[t], c]   (0 outside the image)
//   B[k,n] = W[wt[t]][c][n]  (k-major)   or   W[wt[t]][n][c]  (n-major)
//   output pixel = (i*sout + ph, j*sout + pw) of an [NB,Hout,Wout,Cout] tensor
// Conv2D forward, Conv2DTranspose forward (stride-2 as 4 parity classes), their data gradients and
// the Dense layers are all instances of this one contraction.
// ---------------------------------------------------------------------------------------------
// Tap table of the general kernels (gconv.hip, wgrad.hip): any kernel size up to 5 x 5 (model.py:81-91,121-134 take
// kernels[i] freely).  Entry t = (dh + 8) | (dw + 8) << 4 | weight tap index << 8.
#define DV_MAX_TAPS 25
struct TapTab {
  int n;
  unsigned t[DV_MAX_TAPS];
};

struct GConvParams {
  const float* X;
  const float* W;
  float* U;            // pre-activation / raw output (may be null)
  float* A;            // post-activation output (epi 2) (may be null)
  const float* bias;   // [Cout] or null
  const float* alpha;  // [Hout*Wout*Cout] or null
  int NB, Hin, Win, Cin;
  int Hout, Wout, Cout;
  int Hc, Wc;
  int sin, sout, ph, pw;
  int ntaps;
  TapTab xt;                   // the taps: (dh, dw) source offset and weight tap index of each
  int M, K;
  int w_nmajor;
  int epi;             // 0 raw, 1 +bias, 2 +bias then PReLU (alpha)
  int cin_shift;       // log2(Cin) if power of two else -1
  int dbg;             // 0 normal; >0 timing ablations (wrong results), see gconv.hip
};

int launch_gconv(const GConvParams& p, hipStream_t s);
void debug_set_gconv_tile(int code);  // -1: automatic; code = tile + 100*ablation
int debug_mfma_peak(float* out, int blocks, int iters, int nacc, int randomize, hipStream_t s);

// Second-generation gather-GEMM (gconv2.hip): same contraction, Cin % 32 == 0, all output-parity classes of
// one layer in a single launch.
struct GClass2 {
  int Hc, Wc, M, ph, pw, ntaps, tile0;
  unsigned long long tapcode, wtcode;
};
struct GConv2Params {
  const float* X;
  const float* W;
  float* U;
  float* A;
  const float* bias;
  const float* alpha;
  int NB, Hin, Win, Cin;
  int Hout, Wout, Cout;
  int sin, sout;
  int nclass;
  GClass2 cls[4];
  int w_nmajor;
  int epi;
  int ksplit;          // >1: grid.y K slices, raw partial slabs [ksplit][M][N] written to U
  int batch_major;     // tiles walk (pixel, stamp) instead of (stamp, pixel)
  const float* Uin;    // epi 3: pre-activation of the layer whose output gradient this launch produces
  float* dal_part;     // epi 3: d(alpha) partial slots [slots][alpha_elems] (may be null: no parameter gradients)
  float* db_part;      // epi 3: d(bias) partial rows [m tiles * WGM][Cout] (may be null)
  long alpha_elems;    // Hout*Wout*Cout
  int dbg;             // timing build: phase stamps
  float* dbg_out;
  int prio;            // ablation switch: 4 = one-chunk prefetch with the loads in front of the MFMA block
  unsigned xbytes, wbytes;   // set by launch_gconv2: byte sizes of X and W, the ranges of the gather descriptors
};
// process-wide (development library only, bit 1 of dv_debug_general_kernels): 0 sends gconv2 / gconv_s2 through the select form of
// their gathers instead of the range-checked buffer loads
void debug_set_buffer_gather(int on);
bool buffer_gather_on();
void debug_set_gconv2_dbg(int v, float* out);
void debug_set_gconv2_prio(int v);
int launch_splitk_finish(const float* slabs, int ksplit, long total, int N, const float* bias, const float* alpha,
                         long alpha_per_stamp, float* U, float* A, hipStream_t s);
int launch_gconv2(const GConv2Params& p, hipStream_t s);
// tile geometry the dispatcher will pick (for sizing the epi-3 partial buffers): BM rows, WGM waves along M
void gconv2_tile_geometry(const GConv2Params& p, int* bm, int* wgm, long* mtiles);
void debug_set_gconv2_tile(int code);

// Scene compositing (scene.hip): host float64 buffers in, host float64 buffers out
// device-resident gather + float32 cast (dv_infer_cutouts*, dv_infer_fields*): starts_dev points at the first cutout of the
// chunk, field_dev is field f0 of a stack of fields and sfield_dev[i] the field of cutout i.
int launch_scene_extract_f32(const double* field_dev, int F, int nb, const int* starts_dev, long count, int cs,
                             float* out_dev, hipStream_t s, const int* sfield_dev, int f0);
// compositing of one inference chunk on the device (dv_infer_cutouts_composite, dv_infer_fields_composite): mean / stddev /
// residual fields += the chunk's stamps at integer placements, in object order; per-stamp centre MSE against the field's own
// cutout.  The result pointers are field f0 of a stack, fptr_dev [M + 1] the global stamp number where each field's
// objects begin, the chunk holds stamps obase .. obase + n of fields fy0 .. fy0 + nfields - 1.
// eps_f / eps (both or neither): a third field of the same stack, += the chunk's float32 Monte-Carlo std stamps.
// res2_f (with res_f, without eps_f): a second residual of the same stack, -= the mean stamps like res_f (dv_field_set_pass).
int launch_scene_composite_chunk(double* mean_f, double* std_f, double* res_f, int F, int nb, const float* loc,
                                 const float* scale, const int* places_dev, int n, int cs, hipStream_t s,
                                 const int* fptr_dev, int f0, int fy0, int nfields, long obase, double* eps_f,
                                 const float* eps, double* res2_f = nullptr);
// resident field sets (dv_field_set_pass), stacks of M fields of felems doubles, fptr_dev [M + 1] as above; only
// the fields that have stamps (fptr[m + 1] > fptr[m]) are read or written.
// dst[m] = src[m]
int launch_scene_fields_copy(double* dst_dev, const double* src_dev, const int* fptr_dev, int M, long felems, hipStream_t s);
// out[m] = mean((a[m] - b[m])^2) in float64, summed in a fixed order; part_dev: M * scene_field_mse_blocks(felems) doubles
long scene_field_mse_blocks(long felems);
int launch_scene_field_mse(const double* a_dev, const double* b_dev, const int* fptr_dev, int M, long felems,
                           double* part_dev, double* out_dev, hipStream_t s);
// out[i] = sum(eps_i[:, :, 2]) / sum(loc_i[:, :, 2]) in float64 for the n stamps of a chunk (both device, [n][cs][cs][nb])
int launch_scene_eps_norm(const float* eps, const float* loc, int n, int cs, int nb, double* out_dev, hipStream_t s);
int launch_scene_center_mse(const double* field_dev, int F, int nb, const int* starts_dev, const float* loc, int n, int cs,
                            double* out_dev, hipStream_t s, const int* sfield_dev, int f0);
// the same at fractional positions (dv_infer_fields_fit_composite): objs_dev holds the chunk's placements as
// launch_scene_places derives them from the distances and (fitted) shifts on the device; the chunk goes in sub-chunks in
// object order, each with its B-spline coefficients in coef_dev (scene_frac_coef_doubles, independent of n).
size_t scene_frac_coef_doubles(int cs, int nb, int planes);
size_t scene_frac_obj_bytes(size_t n);
int launch_scene_places(const double* dist_dev, const double* shifts_dev, int n, int F, int cs, void* objs_dev,
                        hipStream_t s);
int launch_scene_composite_frac(double* mean_f, double* std_f, double* res_f, int F, int nb, const float* loc,
                                const float* scale, const void* objs_dev, int n, int cs, hipStream_t s, const int* fptr_dev,
                                int f0, const int32_t* sfield_h, long obase, double* eps_f, const float* eps,
                                double* res2_f, double* coef_dev);
int scene_extract(const double* field_h, int F, int nb, const int32_t* starts_h, int N, int cs, double* out_h,
                  hipStream_t s);
int scene_composite(double* field_h, int F, int nb, const double* stamps_h, const double* pos_h, int N, int cs,
                    double sign, hipStream_t s);
// batched sub-pixel position fit on the r band (posfit.hip): host float64 buffers in and out
int scene_fit_shifts(const double* field_h, int F, const double* stamps_h, int N, int cs, const double* dist_h,
                     double bound, int max_iter, double* shifts_h, double* objective_h, int32_t* iters_h,
                     int32_t* status_h, hipStream_t s);
// the same for M fields [M][F][F]: galaxies field_ptr[m] .. field_ptr[m + 1] are fitted against field m.  Fields are
// uploaded in groups of at most budget_bytes (a single field that needs more is refused).
int scene_fit_shifts_fields(const double* fields_h, int M, int F, const double* stamps_h, const int64_t* field_ptr, int N,
                            int cs, const double* dist_h, double bound, int max_iter, double* shifts_h, double* objective_h,
                            int32_t* iters_h, int32_t* status_h, size_t budget_bytes, hipStream_t s);
// the fit's geometry and launch layout, shared by the calls above and the device-resident stage of
// dv_infer_fields_fit_composite: a plan holds every galaxy's windows; posfit_plan_layout cuts galaxies [a, b) into launches
// (at most max_n galaxies and 1 GiB of workspace each; stamp0 < 0: stamps resident per launch) and returns the first one's
// index; posfit_plan_run runs launches [l0, l1) of an uploaded plan on planes, stamps and [N] result arrays in HBM.
struct PosfitPlan;
int posfit_plan_create(int F, int cs, int N, const double* dist_h, const double* shifts_h, double bound, int max_iter,
                       PosfitPlan** out);
void posfit_plan_destroy(PosfitPlan* p);
struct PosfitPlanFree { void operator()(PosfitPlan* p) const { posfit_plan_destroy(p); } };
using PosfitPlanOwner = std::unique_ptr<PosfitPlan, PosfitPlanFree>;   // a created plan (and its device copy) goes with its scope
int posfit_plan_layout(PosfitPlan* p, int a, int b, int max_n, const int32_t* sfield, int f0, int stamp0);
void posfit_plan_rebase(PosfitPlan* p, int a, int b, int f0);   // fields of [a, b) relative to f0 (laid out with f0 = 0)
int posfit_plan_launch_count(const PosfitPlan* p);
long posfit_plan_work_doubles(const PosfitPlan* p);
size_t posfit_plan_geom_bytes(size_t n);
int posfit_plan_upload(PosfitPlan* p, hipStream_t s);
int posfit_plan_run(const PosfitPlan* p, int l0, int l1, const double* img_dev, const double* total_sq_dev,
                    const double* stamps_dev, double* work_dev, double* shifts_dev, double* objective_dev, int* iters_dev,
                    int* status_dev, hipStream_t s);
// out[f] = sum of squares of plane f of nfields planes of elems doubles; dst[e] = band `band` of pixel e of src [npix][nb]
int launch_posfit_total_sq(const double* img_dev, int nfields, long elems, double* out_dev, hipStream_t s);
int launch_posfit_band_f64(const double* src_dev, long npix, int nb, int band, double* dst_dev, hipStream_t s);
int launch_posfit_band_f32(const float* src_dev, long npix, int nb, int band, double* dst_dev, hipStream_t s);
// catalogue measurement (measure.hip): per-band fluxes and errors and the adaptive moments of band `band` of
// float32 mean / stddev stamps [.][cs][cs][nb]; flux / flux_err [.][nb], shape [.][5] = {r0, c0, Mrr, Mrc, Mcc}, iters and
// status [.].  measure_check: the refusals, before any GPU work.  launch_measure: n stamps in device memory, the output
// pointers at their first row (stddev is read only when flux_err is wanted).  CatRows: the output rows, device or host.
// scene_measure: host arrays, a chunk of stamps on the device at a time (walk_rows, rows.h).
struct CatRows { double *flux, *flux_err, *shape; int *iters, *status; };
int measure_check(const char* who, int cs, int nb, int band, double sigma0, double tol, int max_iter);
int launch_measure(const float* mean_dev, const float* stddev_dev, int n, int cs, int nb, int band, double sigma0,
                   double tol, int max_iter, double* flux_dev, double* flux_err_dev, double* shape_dev, int* iters_dev,
                   int* status_dev, hipStream_t s);
int scene_measure(const float* mean_h, const float* stddev_h, int64_t N, int cs, int nb, int band, double sigma0, double tol,
                  int max_iter, const CatRows& out_h, hipStream_t s);
// the same moments on the observed field with the neighbours subtracted (moments_field.hip): per galaxy the child
// image C = (D - T) + P where the stamp pixel counts (inside the field and, with weights, 0 < W < inf) and P elsewhere; its
// per-band sums and counting pixels, and the adaptive moments of its band plane.  MomentsFieldRows: the output rows, device or
// host - flux / npix [.][nb], shape [.][5], iters, status [.].  launch_moments_field: the complete fields fa .. fz of the view
// v (v.weight null: no mask), the rows counted like its stamps.
// scene_moments_fields: host arrays, whole fields at a time (walk_whole_fields, rows.h); every refusal before GPU work.
size_t measure_lds_bytes(int cs);
// The device view of the stamps of a set of fields, as the kernels that read stamps against fields take it: every per-galaxy
// array - stamps [.][cs][cs][nb], places [.][2], sfield [.] - counts from row 0 of the set, like fptr (the first row of every
// field, and one more); the field stacks [.][F][F][nb] hold the fields from f0 on (data: the observed fields; weight: their
// inverse variances, laid out alike; model: the composited means - each null where the call has none).
// srow, where given: the stamp of row i lies at stamps + srow[i] cs cs nb - a store in another order than the
// call's; only launch_fit_flux_groups reads it, every other table and every output stays indexed by the row of the call.
struct FieldStamps {
  const float* stamps; const int *places, *sfield, *fptr; const double *data, *weight, *model;
  int f0, cs, nb, F;
  const int* srow = nullptr;
};
struct MomentsFieldRows { double* flux; int* npix; double* shape; int *iters, *status; };
int moments_field_rows_check(const char* who, const MomentsFieldRows& o, int64_t n);
int launch_moments_field(const FieldStamps& v, const int* fptr_h, int fa, int fz, int band, double sigma0, double tol,
                         int max_iter, const MomentsFieldRows& rows, hipStream_t s);
int scene_moments_fields(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                         const double* model_h, const double* data_h, const double* weight_h, int M, int F, int band,
                         double sigma0, double tol, int max_iter, const MomentsFieldRows& out_h, int device, hipStream_t s);
// Monte-Carlo catalogue (measure.hip): every sample stamp of a decoder pass measured without a stddev stamp into
// scratch rows, the rows folded per galaxy (Welford, ascending sample order) into means and standard deviations of the nb
// fluxes and of the 8 shape quantities {row, col, Mrr, Mrc, Mcc, sigma, e1, e2}.  McScratch: the rows of one pass (device).
// McState: the results, which also carry the running state between passes ([.][nb], [.][nb], [.][8], [.][8], [.]); the
// per-sample rows [.][S][nb], [.][S][5], [.][S] are given together or not at all.  launch_measure_mc_samples: `rows` stamps
// of a pass.  launch_measure_mc_fold: the pass's n galaxies x reps samples (row r * n + g = sample k0 + r of galaxy g) into
// rows row0 .. of the state; the pass with the last sample writes the standard deviations.  scene_measure_mc: host samples
// [S][N][cs][cs][nb] in, host results (an McState of host pointers) out, a chunk of galaxies on the device at a time.
struct McScratch { double *flux, *shape; int *iters, *status; };
struct McState {
  double *flux_mean, *flux_std, *shape_mean, *shape_std;
  int* n_ok;
  double *sample_flux, *sample_shape;
  int* sample_status;
};
int launch_measure_mc_samples(const float* pass_dev, int rows, int cs, int nb, int band, double sigma0, double tol,
                              int max_iter, const McScratch& w, hipStream_t s);
int launch_measure_mc_fold(const McScratch& w, int n, int reps, int k0, int S, int nb, const McState& st, int64_t row0,
                           hipStream_t s);
int scene_measure_mc(const float* samples_h, int S, int64_t N, int cs, int nb, int band, double sigma0, double tol,
                     int max_iter, const McState& out_h, hipStream_t s);
// blendedness sums (blend.hip): per galaxy {W, A, Bm, Bd} = the sums of g, g P, g T, g D over the stamp pixels
// inside the field, g the Gaussian of the galaxy's adaptive moments; an ineligible row (status not 0 or 2, a non-finite
// shape value, det <= 1e-6) gets four NaN and npix -1.  launch_blend_child: W, A and npix of n stamps in device memory
// (and the NaN of the ineligible rows), every per-galaxy pointer at the first stamp's row.  launch_blend_parent: Bm and Bd
// of n galaxies whose fields are complete: sfield_dev [n] their fields, model_dev / data_dev stacks [.][F][F][nb] that start
// at field f0 (data_dev null: Bd = NaN).  launch_blend_composite_mean: the mean sum of launch_scene_composite_chunk alone
// (the same additions in the same order, so the same bits), for a call that keeps no stddev field.  BlendRows: the output
// rows [.][4], [.], device or host.  scene_blend: host arrays, a chunk of stamps and the fields they span on the device at a
// time (walk_field_rows, rows.h).
struct BlendRows { double* blend; int* npix; };
int blend_check(const char* who, int cs, int nb, int band);
int launch_blend_child(const float* stamps_dev, const double* shape_dev, const int* status_dev, const int* places_dev, int n,
                       int cs, int nb, int band, int F, double* blend_dev, int* npix_dev, hipStream_t s);
int launch_blend_parent(const double* shape_dev, const int* status_dev, const int* places_dev, const int* sfield_dev, int f0,
                        int n, int cs, int nb, int band, int F, const double* model_dev, const double* data_dev,
                        double* blend_dev, hipStream_t s);
int launch_blend_composite_mean(double* mean_f, int F, int nb, const float* loc, const int* places_dev, int n, int cs,
                                const int* fptr_dev, int f0, int fy0, int nfields, long obase, hipStream_t s);
// the end-of-loop sums of a resident field set: per resident row {Bm, Bd, R1, R2} = the sums of g mean, g base,
// g final, g final^2 over the stamp pixels inside the field, against stacks [M][F][F][nb] that start at field 0; base_dev
// null: Bd = NaN; an ineligible row gets four NaN
int launch_blend_set(const double* shape_dev, const int* status_dev, const int* places_dev, const int* sfield_dev, int n, int cs,
                     int nb, int band, int F, const double* mean_dev, const double* base_dev, const double* final_dev,
                     double* sums_dev, hipStream_t s);
int scene_blend(const float* stamps_h, const double* shape_h, const int32_t* status_h, const int32_t* places_h,
                const int64_t* field_ptr, int64_t N, int cs, int nb, int band, const double* model_h, const double* data_h,
                int M, int F, const BlendRows& out_h, hipStream_t s);
// PSF-corrected shapes (regauss.hip): per galaxy the adaptive moments {r', c', Mrr', Mrc', Mcc'} and the kurtosis
// rho4 of the re-Gaussianized band plane, iterations and status (0 / 2 / 3 of the iteration; 4 an ineligible catalogue row,
// 5 no usable PSF, 6 a galaxy its PSF does not resolve: six NaN, 0 iterations).  regauss_check: the refusals, before any GPU
// work.  RegaussPsf: the K PSF images of a call in device memory with their rows - shape [K][5], aux [K][3] = {A_P, FQ,
// rho4}, iters, status - and residuals eps [K][ps][ps]; measure() uploads and measures them on a stream, once per call.
// launch_regauss: n stamps in device memory with their catalogue rows and PSF indices, every per-galaxy pointer at the
// first stamp's row.  RegaussRows: the output rows [.][6], [.], [.], device or host.  scene_regauss: host arrays, a chunk of
// stamps on the device at a time.
struct RegaussRows { double* out; int *iters, *status; };
int regauss_check(const char* who, int cs, int nb, int band, int K, int ps, double psf_sigma0, double tol, int max_iter);
size_t regauss_lds_bytes(int cs, int ps);
struct RegaussPsf {
  DevBuf<double> img, eps, shape, aux;
  DevBuf<int> iters, status;
  static size_t bytes(int K, int ps) { return (size_t)K * ((2 * (size_t)ps * ps + 8) * sizeof(double) + 2 * sizeof(int)); }
  int alloc(int K, int ps);
  int measure(const double* psf_h, int K, int ps, double psf_sigma0, double tol, int max_iter, hipStream_t s);
  int download(int K, double* shape_h, double* aux_h, int32_t* iters_h, int32_t* status_h, hipStream_t s);
};
int launch_regauss(const float* stamps_dev, const double* shape_dev, const int* status_dev, const int* psf_index_dev, int n,
                   int cs, int nb, int band, const RegaussPsf& psf, int K, int ps, double tol, int max_iter, double* out_dev,
                   int* iters_dev, int* ostatus_dev, hipStream_t s);
int scene_regauss(const float* stamps_h, const double* shape_h, const int32_t* status_h, const int32_t* psf_index_h, int64_t N,
                  int cs, int nb, int band, const double* psf_h, int K, int ps, double psf_sigma0, double tol, int max_iter,
                  const RegaussRows& out_h, double* psf_shape_h, double* psf_aux_h, int32_t* psf_iters_h,
                  int32_t* psf_status_h, hipStream_t s);
// aperture photometry (aperture.hip): per galaxy the fluxes, errors and areas of K circular apertures, the Kron
// radius {r1, rho_auto, auto_area}, the flux and error in the automatic ellipse, J flux radii in units of the moment ellipse,
// flags and a status (0; 4 an ineligible catalogue row: every float NaN; 7 no Kron radius: the Kron outputs NaN).
// ApertureParams: dv_aperture_params as the kernel takes it.  ApertureRows: the output rows, device or host - ap_flux / ap_err
// [.][K][nb], ap_area [.][K], flux_auto / auto_err [.][nb], kron [.][3], flux_rho [.][J], flags, status [.]; the two errors are
// null without a stddev stamp.  aperture_check: the refusals, before any GPU work; aperture_rows_check: a missing output.
// launch_aperture: n stamps in device memory with their catalogue rows, every per-galaxy pointer at the first stamp's row.
// scene_aperture: host arrays, a chunk of stamps on the device at a time.
constexpr int AP_MAX_RADII = 8, AP_MAX_FRACTIONS = 4;
struct ApertureParams {
  int K, J, subsample, bisect_iters;
  double radii[AP_MAX_RADII], fractions[AP_MAX_FRACTIONS];
  double kron_factor, kron_min, kron_limit;
};
struct ApertureRows {
  double *ap_flux, *ap_err, *ap_area, *flux_auto, *auto_err, *kron, *flux_rho;
  int *flags, *status;
};
int aperture_check(const char* who, int cs, int nb, int band, const ApertureParams& p);
int aperture_rows_check(const char* who, const ApertureRows& o, const ApertureParams& p, bool err, int64_t n);
size_t aperture_lds_bytes(int cs);
ApertureRows aperture_rows_at(const ApertureRows& o, int64_t r, const ApertureParams& p, int nb);
int launch_aperture(const float* mean_dev, const float* stddev_dev, const double* shape_dev, const int* status_dev, int n, int cs,
                    int nb, int band, const ApertureParams& p, const ApertureRows& rows, hipStream_t s);
int scene_aperture(const float* mean_h, const float* stddev_h, const double* shape_h, const int32_t* status_h, int64_t N, int cs,
                   int nb, int band, const ApertureParams& p, const ApertureRows& out_h, hipStream_t s);
// the same apertures on the fields (aperture.hip): per galaxy the sums of n T, n D and n over the stamp pixels of
// positive count that lie inside the field, T the completed mean field and D the observed field of its field, for the K
// circles and the automatic ellipse of radius kron[1].  ApertureFieldRows: the output rows, device or host - ap_model / ap_data
// [.][K][nb], ap_farea [.][K], auto_model / auto_data [.][nb], auto_farea [.].  launch_aperture_field: n galaxies whose fields
// are complete, every per-galaxy pointer at the first galaxy's row: sfield_dev [n] their fields, model_dev / data_dev stacks
// [.][F][F][nb] that start at field f0 (data_dev null: the data sums are NaN).  scene_aperture_fields: host arrays, a chunk of
// galaxies and the fields they span on the device at a time.
struct ApertureFieldRows { double *ap_model, *ap_data, *ap_farea, *auto_model, *auto_data, *auto_farea; };
int aperture_field_rows_check(const char* who, const ApertureFieldRows& o, const ApertureParams& p, int64_t n);
ApertureFieldRows aperture_field_rows_at(const ApertureFieldRows& o, int64_t r, const ApertureParams& p, int nb);
int launch_aperture_field(const double* shape_dev, const int* status_dev, const double* kron_dev, const int* aper_status_dev,
                          const int* places_dev, const int* sfield_dev, int f0, int n, int cs, int nb, int F,
                          const double* model_dev, const double* data_dev, const ApertureParams& p,
                          const ApertureFieldRows& rows, hipStream_t s);
int scene_aperture_fields(const double* shape_h, const int32_t* status_h, const int32_t* places_h, const int64_t* field_ptr,
                          const double* kron_h, const int32_t* aper_status_h, int64_t N, int cs, int nb, const double* model_h,
                          const double* data_h, int M, int F, const ApertureParams& p, const ApertureFieldRows& out_h,
                          int device, hipStream_t s);
// simultaneous flux fit of the mean stamps of a field to its observed field (fitflux.hip): per band the amplitudes
// a of min |D - sum a_i P_i|^2 over the galaxies of the field, by a dense Cholesky factorisation with dropping.  FitFluxRows: the
// output rows [.][nb], device or host.  fitflux_check / fitflux_plan: every refusal, before any GPU work; the plan is what
// FitFluxWork::alloc takes - the dense scratch (at most scratch_bytes, no more than the fields need) and the pair list.
// launch_fit_flux: the complete fields fa .. fz of a view (FieldStamps above), the rows counted like its stamps; it returns with
// the stream idle.  scene_fit_flux: host arrays, whole fields at a time (walk_whole_fields, rows.h) within half of the device
// memory that is free beside the scratch.  scene_fit_flux_gram: step 1 of one field - the dense G and h to the host.  With weight fields
// (per-pixel inverse variances, a pixel counts iff 0 < W < inf) the sums are weighted, and behind the solve a third
// kernel takes the chi-square of the refitted scene and the count of the counting pixels of every galaxy from a CSR adjacency
// the host builds beside the pair list; without them nothing more is allocated, copied or launched than before.
int scene_fit_flux_gram(const float* stamps_h, const int32_t* places_h, int64_t n, int cs, int nb, const double* data_h, int F,
                        double* gram_h, double* proj_h, int device, hipStream_t s);
constexpr int FF_MAX_N = 1024;                        // galaxies per field (DV_FIT_MAX_N)
struct FitFluxParams { double min_pivot; int64_t scratch_bytes; };
// (chi2, npix: the two rows of the weighted fit, 7s - null in the unweighted one)
// (scale_free, clamped, dual: the three rows of the non-negative fit, 7u - null in the unconstrained one)
struct FitFluxRows {
  double *scale, *var, *gram, *proj; int* status; double* chi2 = nullptr; int* npix = nullptr;
  double* scale_free = nullptr; int* clamped = nullptr; double* dual = nullptr;
};
// The non-negative fit: amplitudes >= 0 by block principal pivoting, at most max_iter factorisations per field and
// band.  iters / status [.][nb]: the per-field outputs, device or host, counted from field 0 of the call like FitFluxSky's.
// on false: the unconstrained fit - nothing more is allocated, copied or launched, and fitflux_solve_kernel runs as before.
struct FitFluxNonneg { bool on = false; int max_iter = 100; int* iters = nullptr; int* status = nullptr; };
// The sky background fitted jointly: q = 1 (a constant) or 3 (a plane) more unknowns per field and band behind
// the galaxies.  FitFluxSky: the per-field outputs, device or host - coef [.][nb][q], cov [.][nb][q][q], status [.][nb][q],
// npix [.][nb] -, counted from field 0 of the call; q = 0: no sky, nothing more is allocated, copied or launched.
struct FitFluxSky { int q = 0; double* coef = nullptr; double* cov = nullptr; int* status = nullptr; long long* npix = nullptr; };
constexpr int FF_SKY_BANDS = 16;                      // (the band limit of the flux fit)
constexpr int FF_SKY_TILE = 4096;                     // pixels of one partial sum of the field sums
inline int fitflux_sky_q(int order) { return order == 0 ? 1 : 3; }
inline size_t fitflux_sky_acc(int q) { return q == 1 ? 3 : 10; }   // K (lower triangle), c, the counting pixels
inline size_t fitflux_sky_tiles(int F) { return ((size_t)F * F + FF_SKY_TILE - 1) / FF_SKY_TILE; }
// (q, sky_part: the sky terms and the doubles of per-tile partial sums of one field, 0 without a sky)
struct FitFluxPlan { size_t scratch_elems = 0, pair_cap = 0, rows = 0; int q = 0; size_t sky_part = 0; };
struct FitFluxWork {
  DevBuf<double> scratch;
  DevBuf<double> sky_part, sky_sums;                  // sky: the partial sums and K, c of the fields of a sub-range
  int q = 0;
  DevBuf<int> pairs;
  DevBuf<long long> foff;
  DevBuf<int> adj_ptr, adj;                           // weighted: the CSR adjacency of a sub-range (rows + 1, <= 2 pairs)
  size_t cap_elems = 0, adj_ptr_cap = 0, adj_cap = 0;   // (elements; the adjacency is never grown behind the plan)
  std::vector<int> pairs_h;                           // host staging of one sub-range
  std::vector<long long> foff_h;
  std::vector<int> adj_ptr_h, adj_h, adj_at_h;
  // what the plan allocates whatever the fields at a time, the sums of one field's sky, and all of it for `fields` fields
  static size_t fixed_bytes(const FitFluxPlan& plan, bool weighted) {
    return plan.scratch_elems * sizeof(double) + plan.pair_cap * 2 * sizeof(int) +
           (weighted ? (plan.pair_cap * 2 + plan.rows + 1) * sizeof(int) : 0);
  }
  static size_t sky_field_bytes(const FitFluxPlan& plan) {
    return plan.q ? (plan.sky_part + FF_SKY_BANDS * fitflux_sky_acc(plan.q)) * sizeof(double) : 0;
  }
  static size_t bytes(const FitFluxPlan& plan, size_t fields, bool weighted) {
    return fixed_bytes(plan, weighted) + fields * sizeof(long long) + (fields ? fields : 1) * sky_field_bytes(plan);
  }
  int alloc(const FitFluxPlan& plan, int64_t max_fields, bool weighted);
};
// The per-field outputs of a fit on the device (the sky's coef, cov, status and npix, the non-negative fit's iters and status),
// for every caller that holds them beside its rows: alloc() for `fields` fields sets `sky` and `nonneg`, the device-side
// structs launch_fit_flux takes (q = 0 / on = false: nothing is allocated); download() queues the copies of nf fields, device
// field dev_f0 on, to field host_f0 on of the caller's arrays.
struct FitFluxFieldOut {
  DevBuf<double> coef, cov;
  DevBuf<int> status, iters, nn_status;
  DevBuf<long long> npix;
  FitFluxSky sky{};
  FitFluxNonneg nonneg{};
  static size_t bytes(int q, bool nonneg, size_t fields, int nb) {
    return fields * nb * ((q ? (size_t)q * (q + 1) * sizeof(double) + q * sizeof(int) + sizeof(long long) : 0) +
                          (nonneg ? 2 * sizeof(int) : 0));
  }
  int alloc(int q, const FitFluxNonneg& nn, size_t fields, int nb);
  int download(const FitFluxSky& sky_h, const FitFluxNonneg& nn_h, size_t host_f0, size_t dev_f0, size_t nf, int nb,
               hipStream_t s) const;
};
int fitflux_check(const char* who, int cs, int nb, int F, const FitFluxParams& p);
int fitflux_rows_check(const char* who, const FitFluxRows& o, int64_t n, bool weighted);
// sky_order -1: no sky; 0 / 1: the bordered systems of 7t, (n + q)^2 doubles per band (F sizes the partial sums)
int fitflux_plan(const char* who, const int64_t* field_ptr, int M, int nb, const FitFluxParams& p, FitFluxPlan* plan,
                 int sky_order, int F);
int fitflux_sky_check(const char* who, int sky_order, const FitFluxSky& o, const FitFluxRows& rows, bool weighted);
// the refusals of the non-negative calls (7u) that need no table: max_iter, the five new outputs, sky outputs given without
// a sky, and (without a sky, where fitflux_sky_check does not run) chi-square outputs that do not match the weights
int fitflux_nonneg_check(const char* who, const FitFluxNonneg& nn, const FitFluxRows& rows, int64_t n, const FitFluxSky& sky,
                         bool weighted);
// v.weight: the weight fields (7s), or null: the unweighted fit.  With weights the chi-square kernel runs behind the solve and
// rows.chi2 / rows.npix are written.  places_h / fptr_h: the host copies of v.places / v.fptr, for the pair list
// sky (7t): q = 1 or 3 sky terms per field and band and the device arrays of their outputs, counted from field 0 of the call; the
// work area must have been planned for the same q.  A sub-range without galaxies is launched when there is a sky
// nn (7u): on - fitflux_nonneg_kernel runs in place of the solve, rows.scale_free / clamped / dual and nn.iters / nn.status
// (device, counted from field 0 of the call) are written; the fields of a sub-range that launches nothing get iters 0, status 0
// solve false: step 1 alone
int launch_fit_flux(const FieldStamps& v, const int32_t* places_h, const int* fptr_h, int fa, int fz, const FitFluxParams& p,
                    FitFluxWork& w, const FitFluxRows& rows, const FitFluxSky& sky, const FitFluxNonneg& nn, bool solve,
                    hipStream_t s);
// What a fit is asked to do, by every caller: the parameters, the host rows, the host weight fields (null: unweighted), the
// order of the sky (-1: none) with its host outputs, the non-negative fit with its, the host rows of the fit by blend groups
// (7w; null: the dense fit), and the name the refusals carry.
struct FitFluxOut {
  FitFluxParams par{}; FitFluxRows rows{}; const double* weights = nullptr; int sky_order = -1; FitFluxSky sky{};
  FitFluxNonneg nonneg{};
  int32_t* group = nullptr; int32_t* group_size = nullptr;
  bool by_groups = false;          // the fit by groups whatever rows were given: a call that refuses missing group rows by name
  const char* who = "dv_scene_fit_flux";
  bool grouped() const { return by_groups || group != nullptr; }
};
// A resident field set as the joint fit of all its passes reads it, in plain pointers.  Device: the stamp store
// [.][cs][cs][nb] with the placement [.][2] and the field [.] of every resident row, and `base`, the fields as uploaded (null: a
// cumulative set, which keeps none).  Host: the placements again, and per kept pass the first row of every field counted from the
// pass's row 0 - what joint_order (rows.h) takes.
struct ResidentRows {
  const float* stamps; const int *places, *field; const double* base;
  const int32_t* places_h; const std::vector<std::vector<int>>& pass_fptr;
  size_t nrows; int M, F, nb, cs;
};
// the regrouping of a resident field set's rows for the joint fit of all passes: destination row d takes the stamp,
// the placement and the field of source row rowmap_dev[d]; n destination rows, every rowmap entry a row the source holds
int launch_fitflux_regroup(const int* rowmap_dev, const float* src, const int* src_places, const int* src_field, int64_t n, int cs,
                           int nb, float* dst, int* dst_places, int* dst_field, hipStream_t s);
int scene_fit_flux(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                   const double* data_h, int M, int F, const FitFluxOut& rq, int device, hipStream_t s);
// The fit by blend groups: the connected components of the overlap graph of every field are found on the GPU and
// each is solved on its own - no limit per field, FF_MAX_N per group, the scratch sum nb n_g^2 doubles.  FitGroupsWork: the
// device tables (counts, scans, pair list, adjacency, labels, group tables, scratch), grown as a call needs them, and their host
// staging.  launch_fit_flux_groups: the complete fields fa .. fz like launch_fit_flux; group_h / gsize_h [.] are HOST rows,
// counted from row 0 of the tables (the host derives them from the labels); field_base: the number of field 0 of the tables in
// the caller's call, for the refusals.  It returns with the stream idle, also when it refuses.  v.stamps null: the groups alone,
// nothing is solved or refused.  lists: when given (null: not wanted), the pair list and the adjacency of the launch are copied out.
struct FitGroupsLists { std::vector<int> pairs, adj_ptr, adj; };
struct FitGroupsWork {
  DevBuf<int> cnt, ptr, pairs, adj, lab, label, rtab, grows;
  DevBuf<long long> gtab;
  DevBuf<double> scratch;
  std::vector<int> label_h, rtab_h, grows_h, gsize_h;
  std::vector<long long> gtab_h;
  // the tables per galaxy beside the scratch: counts, scans, labels, pair list and adjacency, group tables
  static constexpr size_t BYTES_PER_ROW = 12 * sizeof(int) + 4 * sizeof(long long);
};
int launch_fit_flux_groups(const char* who, const FieldStamps& v, const int* fptr_h, int fa, int fz, int field_base,
                           const FitFluxParams& p, FitGroupsWork& w, const FitFluxRows& rows, int32_t* group_h, int32_t* gsize_h,
                           FitGroupsLists* lists, hipStream_t s);
// (rq.group / rq.group_size: the two host rows of the grouping; no sky, no non-negative fit)
int scene_fit_flux_groups(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                          const double* data_h, int M, int F, const FitFluxOut& rq, int device, hipStream_t s);
// The joint fit of all passes of a resident field set: the rows in joint order, the dense fit (7v) on a regrouped copy of the
// stamps or, with rq.grouped(), the fit by blend groups (7y) in place on the store.  rq as the stand-alone calls fill it, its
// rows [nrows][.] in resident-row order; data_h null: the set's base.  Every refusal behind the caller's own, before any GPU work.
int field_set_fit_flux(const ResidentRows& set, const double* data_h, const FitFluxOut& rq, int device, hipStream_t s);
// the blend groups alone, from the placements (no stamps, no fit, no limit on a group), and optionally the pair list and the CSR
// adjacency the fit works from, rows of the call: n_pairs / n_adj are always written, the lists where all three are given
int scene_fit_groups(const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int M, int F, int32_t* group_h,
                     int32_t* gsize_h, int64_t pair_cap, int64_t* n_pairs, int32_t* pairs_h, int64_t adj_cap, int64_t* n_adj,
                     int32_t* adj_ptr_h, int32_t* adj_h, int device, hipStream_t s);
// step 1 of the bordered system of one field (7t): the dense [nb][n + q][n + q] lower triangle and its right-hand side
// [n + q][nb] to the host, the bits the solve starts from
int scene_fit_flux_sky_gram(const float* stamps_h, const int32_t* places_h, int64_t n, int cs, int nb, const double* data_h,
                            const double* weight_h, int F, int sky_order, double* gram_h, double* rhs_h, int device, hipStream_t s);
// the weighted rules of DESIGN 7z: the planes [M][H][W] of a host call (a device source carries its own in DetectDevSrc),
// noise 0 absolute / 1 relative, filter 0 conv / 1 matched, bad_meshes_h [M] nullable
struct DetectWeights {
  const double* weights_h;
  int noise, filter;
  int32_t* bad_meshes_h = nullptr;
};
// the same detector on one band of fields that lie in device memory (dv_field_set_detect): field i of the call is band
// `band` of the [H][W][nb] field number which_h[i] of the stack fields_dev, gathered into the detector's planes on the GPU
struct DetectDevSrc {
  const double* fields_dev;
  int nb, band;
  const int32_t* which_h;
  const double* weights_dev = nullptr;   // (7z) planes [..][H][W] in the stack's numbering, read with a DetectWeights
  const double* planes_dev = nullptr;    // (7za) planes [..][H][W][k] in the stack's numbering, read with a DetectBands
};
// detection on the inverse-variance combination of k bands: the selection, the spectral shape c [k] (null: all
// 1.0), the planes [M][H][W][k] of a host call (null: none; a device source says with has_planes that its planes_dev are
// meant), noise / filter as in DetectWeights, and the outputs only this path has: band_grms_h [M][k], bad_meshes_h [M][k],
// Wt_h [M][H][W], all nullable.  back_h / rms_h of the call are then [M][H][W][k] and the v map (V) comes back through V_h.
struct DetectBands {
  const int32_t* bands;
  int k;
  const double* c;
  const double* planes_h;
  bool has_planes;
  int noise, filter;
  double* band_grms_h = nullptr;
  int32_t* bad_meshes_h = nullptr;
  double* V_h = nullptr;
  double* Wt_h = nullptr;
};
// the argument checks of a DetectBands for fields of nb bands, before any GPU work (who: the caller's name in the message)
int detect_bands_check(const char* who, const int32_t* bands, int k, const double* c, int nb, int noise, int filter);
// the per-object outputs of DESIGN 7zb, all nullable: the integer columns in the order xmin xmax ymin ymax xpeak ypeak
// xvpeak yvpeak flag, the double columns in the order vpeak dflux x_iso y_iso x2 y2 xy, [cap] each and written like the
// catalogue (only when it fits); segmap [M][H][W] is always written
constexpr int DET_OBJ_I = 9, DET_OBJ_D = 7;
struct DetectObjects {
  int32_t* icol[DET_OBJ_I];
  double* dcol[DET_OBJ_D];
  int32_t* segmap_h;
};
// the cleaning pass of DESIGN 7zc: clean_param (beta), and the columns only it has, nullable: nmerged_h, mthresh_h [cap],
// written like the catalogue, and n_raw_h [M], the raw objects of every field, always written
struct DetectClean {
  double clean_param;
  int32_t* nmerged_h;
  double* mthresh_h;
  int64_t* n_raw_h;
};
// the device tables of the cleaning pass over one launch (detect_clean.hip): D and seg of the launch's nf fields of HW pixels,
// rows W wide; per raw object, in catalogue order, rfield (the field in the launch), rbox xmin xmax ymin ymax, rnum (its segmap
// number), rnpix, rd dflux x_iso y_iso x2 y2 xy; per field T and fptr, the first raw object (nf + 1 entries).  Written:
// mthresh [n], der [n][6] a amp alpha cxx cyy cxy, absorber [n], root [2][n] (scratch), rootout [n] the root's raw object,
// newrow [n] the root's row among its field's survivors, nsurv [nf]
struct CleanTables {
  const double* D; const int* seg; int W; long HW; int n, nf;
  const int *rfield, *rbox, *rnum, *rnpix; const double* rd; const double* fT; const int* fptr;
  double *mthresh, *der; int *absorber, *root, *rootout, *newrow, *nsurv;
};
// the four kernels on s; seg is the launch's segmap of px pixels, renumbered in place
int detect_clean_launch(const CleanTables& t, int* seg, long px, int minarea, double beta, hipStream_t s);
// the catalogue of a detection, host arrays: offsets_h [M + 1], globalrms_h [M] and *n_out are always written, the seven
// columns [cap] only when *n_out <= cap (the caller then calls again with cap >= *n_out: the result is deterministic)
struct DetectCatalog {
  int64_t cap; int64_t* n_out; int64_t* offsets_h; double* globalrms_h;
  int32_t *field_h, *parent_h, *npix_h; double *peak_h, *flux_h, *x_h, *y_h;
};
// One detection, as every caller asks for it (detect.hip): M fields of H x W pixels, from the host - fields_h
// [M][H][W] with nb = 0, or interleaved [M][H][W][nb] with a band selection, uploaded as they are and gathered on the GPU - or,
// with dev, from a stack in device memory; par as the C ABI carries it; the modes weights (7z), bands (7za; weights null) and
// objects (7zb), each null when not asked for; the maps [M][H][W], each nullable (with bands back_h and rms_h are
// [M][H][W][k], and V and Wt come back through the DetectBands); the catalogue.
struct DetectRequest {
  const double* fields_h = nullptr; int nb = 0;
  int M = 0, H = 0, W = 0;
  const dv_detect_params* par = nullptr;
  const DetectDevSrc* dev = nullptr;
  const DetectWeights* weights = nullptr; const DetectBands* bands = nullptr; const DetectObjects* objects = nullptr;
  const DetectClean* clean = nullptr;   // (7zc) the cleaning pass; objects may then be null (the catalogue alone)
  double *back_h = nullptr, *rms_h = nullptr, *D_h = nullptr; int32_t* labels_h = nullptr;
  DetectCatalog cat{};
};
int scene_detect(const DetectRequest& rq, hipStream_t s);

// Strip form of the stride-1 3x3 gather-GEMM for the 32-channel high-resolution layers (gconv_strip.hip)
struct GStripParams {
  const float* X;
  const float* W;
  float* U;
  float* A;
  const float* bias;
  const float* alpha;
  const float* zero;   // >= 16 bytes of zeros (source of the out-of-image patch slots)
  int NB, H, Wd, Cin, Cout;
  unsigned long long tapcode, wtcode;   // nine taps: (dh, dw) and weight index, as in GConvParams
  int epi;             // 0 raw, 1 +bias, 2 +bias then PReLU
  int R, patch_floats, strips_per_stamp, nstrips, strips_per_wg;   // filled by the launcher
};
int launch_gconv_strip(GStripParams p, bool nmajor, hipStream_t s);   // 1 = not taken (use gconv2)
int launch_gconv_strip8(GStripParams p, hipStream_t s);               // first layer (Cin 8 -> 32, k-major); 1 = not taken

// Winograd F(2x2, 3x3) form of the stride-1 3x3 layers (wino.hip): X [NB,H,H,Cin] -> [NB,H,H,Cout], pad 1
struct WinoParams {
  const float* X;
  const float* Ut;     // transformed weights [column tile][K chunk][16 pos][32 n][16 k] (wino_weights_kernel)
  float* U;
  float* A;
  const float* bias;
  const float* alpha;
  const float* zero;   // >= 16 bytes of zeros (source of the out-of-image patch slots)
  int NB, H, Cin, Cout;
  int epi;             // 0 raw, 1 +bias, 2 +bias then PReLU
  int nbh, nct, NC, groups, items, items_per_wg;   // filled by the launcher
};
struct WinoWDesc {
  const float* W;      // nine taps, [wt][k][n] or (nmajor) [wt][n][k]
  float* Ut;
  int Cin, Cout, nmajor;
  int wtmap[9];        // weight tap index of the input offset (r - 1, s - 1), r * 3 + s
};
// weight gradient of a stride-1 3x3 layer in the Winograd domain (wino.hip): out[9][Cx][Cy] = sum X (gathered, pad 1) x Y
struct WinoWgradParams {
  const float* X;      // [NB,H,H,Cx]
  const float* Y;      // [NB,H,H,Cy]
  float* part;         // partial slabs [S][16][Cx][Cy]
  size_t part_capacity;
  const float* zero;
  int NB, H, Cx, Cy;
  int nbh, nkt, nnt, nblocks, S, bps;   // filled by the launcher
};
bool wino_wgrad_supported(int NB, int H, int Cx, int Cy);
size_t wino_wgrad_part_floats(int NB, int H, int Cx, int Cy, int* splits_out);
int launch_wino_wgrad(WinoWgradParams p, float* out, hipStream_t s);   // 1 = not taken
int launch_wino_wgrad_finish(const float* part, float* out, int S, int Cx, int Cy, hipStream_t s);
bool wino_supported(int NB, int H, int Cin, int Cout);
size_t wino_weight_floats(int Cin, int Cout);
int launch_wino_weights(const WinoWDesc* descs_dev, const WinoWDesc* descs_host, int n, hipStream_t s);
int launch_wino_conv(WinoParams p, hipStream_t s);   // 1 = not taken

// Stride-2 data-gradient form with the four parity classes fused per workgroup (gconv_s2.hip).
// Class c = 2*[row parity has two taps] + [column parity has two taps]; neighbour e = 2*[dh == x] + [dw == x].
struct GConvS2Params {
  const float* X;
  const float* W;      // n-major taps: W[wt][n][k]
  float* U;
  float* A;
  const float* bias;
  const float* alpha;
  int NB, Hin, Win, Cin;
  int Hout, Wout, Cout;
  int Hc, Wc, M;       // base grid (ceil(Hout/2)) and NB*Hc*Wc
  int epi;             // 0 raw, 1 +bias, 2 +bias then PReLU
  int ndh[4], ndw[4];  // source offset of neighbour e
  int cph[4], cpw[4];  // output parity of class c
  int wt[4][4];        // weight tap index of (neighbour e, class c); unused pairs 0
  unsigned* dbg_out;   // per-workgroup timeline stamps (tuning aid) or null
  unsigned xbytes, wbytes;   // set by launch_gconv_s2: byte sizes of X and W, the ranges of the gather descriptors
};
int launch_gconv_s2(const GConvS2Params& p, hipStream_t s);
void debug_set_gconv_s2_tile(int code);
void debug_set_wino_variant(int v);   // 1: eight-wave Winograd conv kernel, 2: four-wave pipelined one (default)
void debug_set_gconv_s2_dbg(unsigned* out);

// ---------------------------------------------------------------------------------------------
// Weight gradient: dW[(t, cx), cy] = sum_p Xg[p, t][cx] * dY[p][cy], split over pixel ranges into
// partial slabs [nsplit][9*Cx][Cy] that reduce_partials() sums in a fixed order (deterministic).
// ---------------------------------------------------------------------------------------------
struct WGradParams {
  const float* X;     // gathered side [NB,Hx,Wx,Cx]
  const float* Y;     // dense side    [NB,Hy,Wy,Cy]
  float* part;        // [nsplit][rows_total][Cy]
  int NB, Hx, Wx, Cx;
  int Hy, Wy, Cy;
  int Hc, Wc, sx, sy, ph, pw;
  int ntaps;
  TapTab xt;          // the taps (dh, dw, weight tap index)
  int P;              // NB*Hc*Wc
  int rows_total;     // ntaps*Cx (slab rows; launch covers rows wt*Cx..)
  int nsplit;
  int pchunk;         // pixels per split (multiple of 32)
  // filled by launch_wgrad: exact division of a pixel index by Hc*Wc and by Wc as multiply-high + shifts (the gather
  // decodes its pixel once per chunk and thread; a 32-bit division is ~35 vector instructions, this is 5 - and on
  // gfx950 every vector instruction is fp32-MFMA time)
  unsigned div_hw_m, div_hw_s1, div_hw_s2, div_w_m, div_w_s1, div_w_s2;
};
int launch_wgrad(const WGradParams& p, hipStream_t s);
// Dense kernel gradient G[i][j] = sum_b X[b][i] * Y[b][j] (fp32 rows X [NB][ldx], Y [NB][ldy]; Dense layers of the trunk,
// model.py:96-98,114-117): one pass, written once, no slabs (wgrad.hip, round 6)
int launch_dense_wgrad_tn(const float* X, int ldx, const float* Y, int ldy, int NB, int I, int J, float* G, int ldg,
                          hipStream_t s);

// Strip form for the high-resolution few-channel layers (wgrad_strip.hip)
struct WStripParams {
  const float* X;
  const float* Y;
  float* part;
  size_t part_capacity;   // floats available in `part`
  int NB, Hx, Wx, Hy, Wy;
  int pb;
  const float* zero;      // >= 16 bytes of zeros in device memory (source of out-of-image LDS-DMA pieces)
  int R, XR, xs_floats, ys_floats, strips_per_stamp, nstrips, strips_per_wg;   // filled by the launcher
  int dbg;                // timing ablations (wrong results), bit flags: 1 no refill DMA, 2 no MFMA, 4 phase stamps, 8 MFMA only
  // first-layer form only (Cx = 8): fuse the PReLU backward of the layer's output.  Y is then d(activation).
  const float* U;         // pre-activation [NB,Hy,Wy,32]; null: Y already is d(pre-activation)
  const float* alpha;     // PReLU slopes [Hy,Wy,32]
  float* dal_part;        // d(alpha) partials [groups][Hy*Wy*32]
  float* db_part;         // d(bias) partials [workgroups][32]
  size_t dal_capacity, db_capacity;   // floats available in dal_part / db_part
  long alpha_elems;       // Hy*Wy*32
  int groups;             // filled by the launcher
  int* groups_out;        // host: number of d(alpha) partial slabs written
};
bool wgrad_strip8_fusable(int Hy, int Wy);
void debug_set_strip(int v);
bool wgrad_strip_supported(int Cx, int Cy, int sx, int ntaps);
int launch_wgrad_strip(const WStripParams& p, int Cx, int Cy, int sx, hipStream_t s, int* nsplit_out);

// out[(r/Cpad)*Creal + r%Cpad][c] = scale * sum_s part[s][r][c]   for r%Cpad < Creal
// the slab reductions of a whole backward pass in one launch: entry i sums nsplit slabs of slab4 float4 elements
// ([rows][ncols4] each) into out, rows compacted from cpad to creal channels like launch_reduce_partials
#define DV_WRED_MAX 24
struct WRedEntry {
  const float* part;
  float* out;
  int nsplit, slab4, ncols4, cpad, creal;
};
struct WRedBatch {
  WRedEntry e[DV_WRED_MAX];
  int count;
};
int launch_reduce_partials_batch(const WRedBatch& b, hipStream_t s);
int launch_reduce_partials(const float* part, float* out, int nsplit, long slab_elems, int ncols, int cpad,
                           int creal, hipStream_t s);

// pointwise / reduction kernels -----------------------------------------------------------------
struct HeadParams {
  const float* tpre;   // [NB,Hd,Hd,2*nb] head conv output before relu
  const float* y;      // dataset labels [*,H,H,nb] (null: no loss)
  const int* idx;      // per-stamp dataset row (null: first + b)
  int first;
  float* dt;           // [NB,Hd,Hd,2*nb] gradient wrt tpre (null: none)
  float* loc;          // [NB,H,H,nb] or null
  float* scale;        // [NB,H,H,nb] or null
  float* part;         // [nblocks][2] partial sums (nll, squared error)
  int NB, Hd, H, nb, crop0;
  int ld;              // channels per pixel row of tpre / dt (2*nb, or padded to 16)
  float sigma_floor;
  float gscale;        // 1/(Bglobal*H*H*nb)
  // Keras' "mse" metric of the reference compares the labels with a SAMPLE of the output distribution (model.py:158
  // convert_to_tensor_fn = sample, train.py:128): with mse_sample the squared error is taken against
  // loc + sigma * eps, eps(stamp b, element e) = Philox4x32-10(counter (b, e / 4, mse_stream, 0), key mse_seed), e the
  // element index inside the [H,H,nb] stamp (oracle: vae_oracle.philox_normal(seed, stream, B, H*H*nb))
  int mse_sample;
  int mse_row0;        // index of this launch's first stamp inside the rank's batch (forward lanes)
  unsigned mse_stream;
  unsigned long long mse_seed;
};
#define DV_MSE_STREAM 0x4D534500u   /* + rank */
int launch_head(const HeadParams& p, hipStream_t s, int* nblocks_out);

// input BatchNorm: the per-band state / sum rows are DV_BN_MAXC wide (bands 1 .. 15: the folded first conv reads bands + 1
// channels of an 8- or 16-channel row)
constexpr int DV_BN_MAXC = 16;
int launch_bn_stats(const float* x, const int* idx, int first, int NB, int HW, int C, float* part, int* nblocks,
                    hipStream_t s);
// out[c] = scale * sum_r part[r*ld + c] for c < ncols (ld = row stride, 0: ncols)
int launch_reduce_rows_f64(const float* part, int nrows, int ncols, float* out, float scale, hipStream_t s,
                           int ld = 0);
// bnstate: [0..C) scale, [C..2C) shift, [2C..3C) mean, [3C..4C) inv_std
int launch_bn_finalize(const float* sums, float count, int C, const float* gamma, const float* beta,
                       float* moving_mean, float* moving_var, float eps, float momentum, int unbiased,
                       int training, int update_moving, float* bnstate, hipStream_t s);
int launch_bn_apply(const float* x, const int* idx, int first, int NB, int HW, int C, int Cpad, const float* bnstate,
                    float* xn, hipStream_t s);
int launch_prelu_fwd(const float* u, const float* alpha, float* a, long NB, int E, hipStream_t s);
// da -> du in place; dalpha partials [nsplit][E]; dbias partials (mode by HW): see pointwise.hip
int launch_prelu_bwd(float* da, const float* u, const float* alpha, int NB, int E, int C, int nsplit,
                     float* dalpha_part, float* dbias_part, int* dbias_rows, hipStream_t s);
int launch_colsum(const float* x, long rows, int C, float* part, int* nrows_part, hipStream_t s);
// out[b][n] = sum_k x[b][k] * W[n][k], N <= 64 (one wave per row)
int launch_dense_narrow(const float* x, const float* W, float* out, int NB, int K, int N, hipStream_t s);


struct SamplerParams {
  const float* t;      // [NB, d + d(d+1)/2]
  float* eps;          // [NB, d] (read; written first when gen != 0)
  float* z;            // [NB, d]
  float* kl;           // [NB]
  float* stddev;       // [NB, d] or null
  int NB, d;
  int ldt, ldz;        // row strides of t and of eps / z / stddev (>= d + d(d+1)/2 and >= d; pad columns are written as zeros)
  float diag_shift;
  int gen;             // 1: generate eps with Philox(seed, stream, row0 + b)
  unsigned long long seed;
  unsigned stream;
  unsigned row0;
  int rep_nb;          // > 0: row r is Monte-Carlo sample r / rep_nb of stamp r % rep_nb (seed + sample, t row of the stamp)
  const unsigned long long* seed_ptr;   // non-null: the seed is read from device memory (replayed hipGraphs)
  // nslab > 0 (bf16 engine, btrunk.hip): the encoder Dense arrives as K-split partial sums; the row is
  // t[b][i] = tbias[i] + sum_s slab[s][b][i] (added in order), formed here and also written to `t_out` (same strides as
  // t, pad columns zero) for the backward pass and the API - the finish launch of the split product is this kernel
  const float* slab;   // [nslab][*][lds]
  const float* tbias;  // [d + d(d+1)/2]
  float* t_out;
  long slab_stride;
  int nslab, lds;
  // non-null: the PReLU in front of the decoder's first Dense (model.py:113) is applied here as well,
  // ain[b][i] = z > 0 ? z : alpha_in[i] * z (row stride ldz, pad columns zero) - one launch less on the forward chain
  const float* alpha_in;
  float* ain;
};
int launch_sampler_fwd(const SamplerParams& p, hipStream_t s);
// ldt: row stride of t and dt, ldz: of eps, z and dz (pad columns of dt are written as zeros)
int launch_sampler_bwd(const float* t, const float* eps, const float* z, const float* dz, float* dt, int NB, int d,
                       int ldt, int ldz, float diag_shift, float kls, hipStream_t s);
// the same two for latent_dim > 64 (one workgroup per stamp, any d; same arguments and semantics, the KL sum in another
// fixed order)
int launch_sampler_wide_fwd(const SamplerParams& p, hipStream_t s);
int launch_sampler_wide_bwd(const float* t, const float* eps, const float* z, const float* dz, float* dt, int NB, int d,
                            int ldt, int ldz, float diag_shift, float kls, hipStream_t s);

int launch_adam(float* w, float* m, float* v, const float* g, long n, float lr_t, float b1, float b2, float eps,
                hipStream_t s);
int launch_pad_w1(const float* w, const float* gamma, const float* beta, float* wp, int taps, int cin, int cpad,
                  int cout, hipStream_t s);
int launch_bn_conv0_grads(const float* G, const float* w, const float* gamma, const float* beta, float* dW,
                          float* dgamma, float* dbeta, int taps, int cin, int cpad, int cout, hipStream_t s);
int launch_fill(float* p, long n, float v, hipStream_t s);
int launch_normalise(float* x, long n, bool inverse, hipStream_t s);
int launch_welford_update(const float* x, float* mean, float* m2, long n, int k, hipStream_t s);
int launch_welford_finish(float* m2, long n, int count, hipStream_t s);
// x holds `reps` consecutive blocks of n elements (samples k0 .. k0+reps-1 of the same n statistics), folded in order
int launch_welford_update_multi(const float* x, float* mean, float* m2, long n, int reps, int k0, hipStream_t s);
int launch_pad_cols(const float* src, float* dst, int rows, int nsrc, int ndst, hipStream_t s);
int launch_take_cols(const float* src, float* dst, int rows, int nsrc, int ndst, hipStream_t s);
int launch_gather_rows(const float* src, const int* idx, int first, int NB, long row_elems, float* dst,
                       hipStream_t s);


// ---- scalar-base LDS-DMA (device code only) -------------------------------------------------------------------
// fp32 MFMA and the vector ALU are the same lanes on gfx950 (the fp32 matrix peak IS the vector peak), so every vector
// instruction a wave issues - including the address selects in front of a gather - is time its MFMA stream does not get.
// These helpers issue one 1-KiB global_load_lds piece whose address is a SCALAR base plus a 32-bit lane offset that can be
// a kernel-long constant; lanes that must read zeros (outside the image) are switched by an execution mask, which costs one
// compare per piece instead of a 64-bit select.  All lanes of the wave must be active at the call.
#if defined(__HIPCC__)
// one 1-KiB LDS-DMA piece, address = scalar base + 32-bit lane offset; the lanes outside `m_dma` (of the first 16 lanes
// when LAST16: the piece that ends a buffer) get 16 bytes of the zero page instead
__device__ __forceinline__ void dv_dma_exec(unsigned lds, unsigned voff, const void* sbase, unsigned long long mask);
template <bool LAST16>
__device__ __forceinline__ void dv_dma_masked(unsigned lds, unsigned voff, const void* sbase, unsigned long long m_dma,
                                              unsigned vnull, const void* zero) {
  dv_dma_exec(lds, voff, sbase, m_dma);
  const unsigned long long m_zero = LAST16 ? (~m_dma & 0xffffull) : ~m_dma;
  if (m_zero) dv_dma_exec(lds, vnull, zero, m_zero);   // (scalar branch: interior pieces issue one instruction)
}
// one LDS-DMA piece for the lanes of `mask` only (the other lanes' slots keep what they hold)
__device__ __forceinline__ void dv_dma_exec(unsigned lds, unsigned voff, const void* sbase, unsigned long long mask) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_mov_b64 exec, %1\n\t"
      "global_load_lds_dwordx4 %2, %3\n\t"
      "s_mov_b64 exec, -1"
      :
      : "s"(lds), "s"(mask), "v"(voff), "s"(sbase)
      : "memory");
}
__device__ __forceinline__ void dv_dma(unsigned lds, unsigned voff, const void* sbase) {
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2"
      :
      : "s"(lds), "v"(voff), "s"(sbase)
      : "memory");
}
#endif

}  // namespace dv
