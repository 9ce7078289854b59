// Adaptive moments on the observed field with the neighbours subtracted: the measurement of 7j on the child
// image of every galaxy instead of on the network's own mean stamp.
//
// Per galaxy i of field m (P_i the mean stamp [cs][cs][nb] float32 at place (pr, pc), T the completed mean field and D the
// observed field [F][F][nb] float64, W an optional weight field of the same shape):
//   stamp pixel (r, c), band b lies on field pixel (R, Cc) = (pr + r, pc + c); it COUNTS iff it lies inside the field and,
//   with W, 0 < W[R, Cc, b] < inf (the rule of 7s)
//   C_i[r, c, b] = (D[R, Cc, b] - T[R, Cc, b]) + (double)P_i[r, c, b]   where the pixel counts (two roundings, that order)
//                = (double)P_i[r, c, b]                                  elsewhere: the model fills in what is hidden
//   flux_data[b] = sum C_i[., ., b]   npix_data[b] = the counting pixels
//   shape_data, iters_data, status_data = ms_iterate on C_i[:, :, band] from the stamp centre and sigma0^2 I
// With D == T bit for bit C_i is P_i, and every output has the bits of measure_kernel on the same stamp.
//
// One workgroup of 256 threads per galaxy, float64.  Thread t takes the stamp pixels e = t + 256 k like measure_stamp, so the
// per-band sums are reduced in its order; for its pixel it reads the nb consecutive floats of P and the nb consecutive doubles
// of D, T and W: a wave reads 64 nb consecutive doubles of a field row (broken where a stamp row ends), never one band plane
// strided through the field.  The band plane goes to LDS by the thread that ms_iterate reads it from.  No atomics.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>

namespace dv {

namespace {
constexpr int MF_MAX_BANDS = 16;

__device__ __forceinline__ bool mf_counts(double w) { return w > 0.0 && w < __longlong_as_double(0x7ff0000000000000LL); }

// (D - T) + P: two roundings in that order
__device__ __forceinline__ double mf_child(double d, double t, double p) {
#pragma clang fp contract(off)
  const double res = d - t;
  return res + p;
}

// stamps / places / sfield and the five outputs at the first galaxy's row; model / data / weight stacks [.][F][F][nb] that
// start at field f0
template <bool MASKED>
__global__ __launch_bounds__(MS_THREADS) void moments_field_kernel(const float* __restrict__ stamps, const int* __restrict__ places,
                                                                   const int* __restrict__ sfield, int f0, int cs, int nb, int band,
                                                                   int F, const double* __restrict__ model,
                                                                   const double* __restrict__ data, const double* __restrict__ weight,
                                                                   double sigma0, double tol, int max_iter, double* __restrict__ flux,
                                                                   int* __restrict__ npix, double* __restrict__ shape,
                                                                   int* __restrict__ iters, int* __restrict__ status) {
  extern __shared__ double s_mem[];
  const long gi = blockIdx.x;
  const int np = cs * cs;
  double* plane = s_mem;                    // [cs][cs]
  double* s_red = s_mem + np;               // [MS_RED]
  const float* P = stamps + gi * np * nb;
  const int pr = places[2 * gi], pc = places[2 * gi + 1];
  const long fbase = (long)(sfield[gi] - f0) * F * F * nb;

  double f[MF_MAX_BANDS];
  int cnt[MASKED ? MF_MAX_BANDS : 1];
#pragma unroll
  for (int b = 0; b < MF_MAX_BANDS; ++b) f[b] = 0.0;
#pragma unroll
  for (int b = 0; b < (MASKED ? MF_MAX_BANDS : 1); ++b) cnt[b] = 0;
  const int step_r = MS_THREADS / cs, step_c = MS_THREADS - step_r * cs;
  int r = threadIdx.x / cs, c = threadIdx.x - r * cs;
  for (int e = threadIdx.x; e < np; e += MS_THREADS) {
    const float* p = P + (long)e * nb;
    const int R = pr + r, Cc = pc + c;
    const bool in = (unsigned)R < (unsigned)F && (unsigned)Cc < (unsigned)F;
    const long o = in ? fbase + ((long)R * F + Cc) * nb : 0;   // (read only where the pixel lies inside the field)
#pragma unroll
    for (int b = 0; b < MF_MAX_BANDS; ++b) {
      if (b < nb) {
        double v = (double)p[b];
        bool on = in;
        if (MASKED && in) on = mf_counts(weight[o + b]);
        if (on) v = mf_child(data[o + b], model[o + b], v);
        if (MASKED) cnt[MASKED ? b : 0] += on ? 1 : 0;
        f[b] += v;
        if (b == band) plane[e] = v;
      }
    }
    c += step_c;
    r += step_r;
    if (c >= cs) { c -= cs; ++r; }
  }
  // without a mask the counting pixels are the clipped rectangle, the same in every band
  const int rows_in = max(0, min(pr + cs, F) - max(pr, 0)), cols_in = max(0, min(pc + cs, F) - max(pc, 0));
#pragma unroll
  for (int b = 0; b < MF_MAX_BANDS; ++b) {
    if (b < nb) {                           // (nb is uniform: every thread takes the same barriers)
      if (MASKED) {
        double a[2] = {f[b], (double)cnt[MASKED ? b : 0]};   // (a count of at most 8100: exact in a double)
        ms_block_sum<2>(a, s_red);
        if (threadIdx.x == 0) {
          flux[gi * nb + b] = a[0];
          npix[gi * nb + b] = (int)a[1];
        }
      } else {
        double a[1] = {f[b]};
        ms_block_sum<1>(a, s_red);
        if (threadIdx.x == 0) {
          flux[gi * nb + b] = a[0];
          npix[gi * nb + b] = rows_in * cols_in;
        }
      }
    }
  }
  // (every thread reads back only the plane elements it wrote itself: the loop above and ms_iterate walk the same e)

  const double ctr = 0.5 * (double)(cs - 1);
  double r0 = ctr, c0 = ctr, Mrr = sigma0 * sigma0, Mrc = 0.0, Mcc = sigma0 * sigma0;
  int it = 0, st = 2;
  ms_iterate(plane, cs, tol, max_iter, r0, c0, Mrr, Mrc, Mcc, it, st, s_red);
  if (threadIdx.x == 0) {
    double* sh = shape + gi * 5;
    sh[0] = r0;
    sh[1] = c0;
    sh[2] = Mrr;
    sh[3] = Mrc;
    sh[4] = Mcc;
    iters[gi] = it;
    status[gi] = st;
  }
}
}  // namespace

int moments_field_rows_check(const char* who, const MomentsFieldRows& o, int64_t n) {
  if (n > 0 && (!o.flux || !o.npix || !o.shape || !o.iters || !o.status)) {
    set_error("%s: flux_data, npix_data, shape_data, iters_data and status_data must all be given", who);
    return E_INVALID;
  }
  return OK;
}

void moments_field_columns(Rows& r, MomentsFieldRows& dev, const MomentsFieldRows& host, int nb) {
  r.add(dev.flux, host.flux, nb);
  r.add(dev.npix, host.npix, nb);
  r.add(dev.shape, host.shape, 5);
  r.add(dev.iters, host.iters, 1);
  r.add(dev.status, host.status, 1);
}

// The complete fields fa .. fz of a call: every per-galaxy device array counts from row 0 of the call, like fptr_h (the first
// row of every field); the field stacks hold the fields from f0 on.  weight_dev null: no mask.
int launch_moments_field(const float* stamps_dev, const int* places_dev, const int* sfield_dev, const double* model_dev,
                         const double* data_dev, const double* weight_dev, int f0, const int* fptr_h, int fa, int fz, int cs,
                         int nb, int band, int F, double sigma0, double tol, int max_iter, const MomentsFieldRows& rows,
                         hipStream_t s) {
  if (fz < fa) return OK;
  const size_t r0 = (size_t)fptr_h[fa];
  const int n = fptr_h[fz + 1] - fptr_h[fa];
  if (n <= 0) return OK;
  const float* st = stamps_dev + r0 * cs * cs * nb;
  const int *pl = places_dev + 2 * r0, *sf = sfield_dev + r0;
  double *fl = rows.flux + r0 * nb, *sh = rows.shape + r0 * 5;
  int *np = rows.npix + r0 * nb, *it = rows.iters + r0, *stt = rows.status + r0;
  if (weight_dev)
    hipLaunchKernelGGL(moments_field_kernel<true>, dim3((unsigned)n), dim3(MS_THREADS), measure_lds_bytes(cs), s, st, pl, sf, f0, cs,
                       nb, band, F, model_dev, data_dev, weight_dev, sigma0, tol, max_iter, fl, np, sh, it, stt);
  else
    hipLaunchKernelGGL(moments_field_kernel<false>, dim3((unsigned)n), dim3(MS_THREADS), measure_lds_bytes(cs), s, st, pl, sf, f0, cs,
                       nb, band, F, model_dev, data_dev, weight_dev, sigma0, tol, max_iter, fl, np, sh, it, stt);
  DV_HIP(hipGetLastError());
  return OK;
}

// host arrays in, host rows out, whole fields at a time: as many consecutive fields as half of free device memory holds with
// their stamps, tables and rows
int scene_moments_fields(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                         const double* model_h, const double* data_h, const double* weight_h, int M, int F,
                         int band, double sigma0, double tol, int max_iter, const MomentsFieldRows& out_h, int device,
                         hipStream_t s) {
  const char* who = "dv_scene_moments_fields";
  DV_TRY(measure_check(who, cs, nb, band, sigma0, tol, max_iter));
  if (N < 0 || M < 0 || !field_ptr || (N > 0 && (!stamps_h || !places_h || !model_h || !data_h))) {
    set_error("%s: stamps, places, field_ptr, model_fields and data_fields must all be given", who);
    return E_INVALID;
  }
  DV_TRY(moments_field_rows_check(who, out_h, N));
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, nullptr, nullptr));   // (the chunks build their own tables)
  if (N == 0) return OK;
  MomentsFieldRows d{};
  Rows out;
  moments_field_columns(out, d, out_h, nb);
  const size_t stamp = (size_t)cs * cs * nb, felems = (size_t)F * F * nb;
  const size_t per_stamp = stamp * sizeof(float) + 3 * sizeof(int) + out.bytes();
  const size_t per_field = (weight_h ? 3 : 2) * felems * sizeof(double);
  DV_HIP(hipSetDevice(device));
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 2;
  // the chunks: consecutive fields, as many as fit (at least one)
  std::vector<int> cuts{0};
  size_t cmax_s = 0, cmax_f = 0;
  for (int f = 0; f < M;) {
    size_t bytes = 0;
    int g = f;
    while (g < M) {
      const size_t add = (size_t)(field_ptr[g + 1] - field_ptr[g]) * per_stamp + per_field;
      if (g > f && bytes + add > budget) break;
      bytes += add;
      ++g;
    }
    if (bytes > budget) {
      set_error("%s: field %d with its %ld stamps needs %zu bytes of device memory, %zu are available", who, f,
                (long)(field_ptr[f + 1] - field_ptr[f]), bytes, budget);
      return E_NOMEM;
    }
    cmax_s = std::max(cmax_s, (size_t)(field_ptr[g] - field_ptr[f]));
    cmax_f = std::max(cmax_f, (size_t)(g - f));
    cuts.push_back(g);
    f = g;
  }
  DevBuf<float> stamps;
  DevBuf<double> model, data, wdata;
  DevBuf<int> places, sf;
  DV_TRY(stamps.alloc(cmax_s * stamp));
  DV_TRY(places.alloc(cmax_s * 2));
  DV_TRY(sf.alloc(cmax_s));
  DV_TRY(model.alloc(cmax_f * felems));
  DV_TRY(data.alloc(cmax_f * felems));
  if (weight_h) DV_TRY(wdata.alloc(cmax_f * felems));
  DV_TRY(out.alloc((int64_t)cmax_s));
  std::vector<int> sf_h, fptr_h;
  StreamDrain drain(s);
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    const int fa = cuts[k], fz = cuts[k + 1];          // fields fa .. fz - 1, their rows counted from the chunk's first
    const int64_t r0 = field_ptr[fa], n = field_ptr[fz] - r0;
    if (n == 0) continue;
    fptr_h.assign((size_t)(fz - fa) + 1, 0);
    sf_h.assign((size_t)n, 0);
    for (int f = fa; f < fz; ++f) {
      fptr_h[(size_t)(f - fa) + 1] = (int)(field_ptr[f + 1] - r0);
      for (int64_t i = field_ptr[f]; i < field_ptr[f + 1]; ++i) sf_h[(size_t)(i - r0)] = f - fa;
    }
    const size_t fbytes = (size_t)(fz - fa) * felems * sizeof(double), foff = (size_t)fa * felems;
    DV_HIP(hipMemcpyAsync(stamps, stamps_h + (size_t)r0 * stamp, (size_t)n * stamp * sizeof(float), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(places, places_h + (size_t)r0 * 2, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(sf, sf_h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(model, model_h + foff, fbytes, hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(data, data_h + foff, fbytes, hipMemcpyHostToDevice, s));
    if (weight_h) DV_HIP(hipMemcpyAsync(wdata, weight_h + foff, fbytes, hipMemcpyHostToDevice, s));
    DV_TRY(launch_moments_field(stamps, places, sf, model, data, weight_h ? wdata.get() : nullptr, 0, fptr_h.data(), 0,
                                fz - fa - 1, cs, nb, band, F, sigma0, tol, max_iter, d, s));
    DV_TRY(out.download(r0, n, s));
    DV_HIP(hipStreamSynchronize(s));                   // the device buffers and the host tables are reused by the next chunk
  }
  drain.dismiss();
  return OK;
}

}  // namespace dv
