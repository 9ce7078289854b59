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

// The complete fields fa .. fz of the view v: the rows count from row 0 of the set like its stamps, fptr_h is the host copy of
// v.fptr.  v.weight null: no mask.
int launch_moments_field(const FieldStamps& v, const int* fptr_h, int fa, int fz, int band, double sigma0, double tol,
                         int max_iter, const MomentsFieldRows& rows, hipStream_t s) {
  if (fz < fa) return OK;
  const size_t r0 = (size_t)fptr_h[fa];
  const int n = fptr_h[fz + 1] - fptr_h[fa], cs = v.cs, nb = v.nb;
  if (n <= 0) return OK;
  const float* st = v.stamps + r0 * cs * cs * nb;
  const int *pl = v.places + 2 * r0, *sf = v.sfield + r0;
  double *fl = rows.flux + r0 * nb, *sh = rows.shape + r0 * 5;
  int *np = rows.npix + r0 * nb, *it = rows.iters + r0, *stt = rows.status + r0;
  if (v.weight)
    hipLaunchKernelGGL(moments_field_kernel<true>, dim3((unsigned)n), dim3(MS_THREADS), measure_lds_bytes(cs), s, st, pl, sf, v.f0,
                       cs, nb, band, v.F, v.model, v.data, v.weight, sigma0, tol, max_iter, fl, np, sh, it, stt);
  else
    hipLaunchKernelGGL(moments_field_kernel<false>, dim3((unsigned)n), dim3(MS_THREADS), measure_lds_bytes(cs), s, st, pl, sf, v.f0,
                       cs, nb, band, v.F, v.model, v.data, v.weight, sigma0, tol, max_iter, fl, np, sh, it, stt);
  DV_HIP(hipGetLastError());
  return OK;
}

// host arrays in, host rows out, whole fields at a time (walk_whole_fields): the stamps, tables, rows and the two or three
// field stacks of a run of fields
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
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, nullptr, nullptr));   // (the walker builds its own tables)
  if (N == 0) return OK;
  FieldStamps v{};
  v.cs = cs, v.nb = nb, v.F = F;
  MomentsFieldRows d{};
  Rows in, out;
  in.add(v.stamps, stamps_h, (size_t)cs * cs * nb);
  in.add(v.places, places_h, 2);
  moments_field_columns(out, d, out_h, nb);
  WholeFields f{model_h, data_h, weight_h, 0, 0, 0, false};
  DV_HIP(hipSetDevice(device));
  return walk_whole_fields(who, M, field_ptr, N, f, v, in, out, s, [&](const FieldStamps& run, int, int nf, int64_t, const int* fptr_h) {
    return launch_moments_field(run, fptr_h, 0, nf - 1, band, sigma0, tol, max_iter, d, s);
  });
}

}  // namespace dv
