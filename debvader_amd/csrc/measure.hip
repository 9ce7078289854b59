// Catalogue measurement of deblended galaxies: per-band fluxes and their errors, and the adaptive moments
// of one band, for every stamp of a batch.  The reference ships an empty debvader.measure package; the measurement is
// defined here.
//
// Per stamp, float64 throughout (P = the network's mean stamp [cs][cs][nb], S = its stddev stamp, float32 widened):
//   flux[b]     = sum P[r, c, b]                flux_err[b] = sqrt(sum S[r, c, b]^2)
//   adaptive moments of I = P[:, :, band]: from r0 = c0 = (cs - 1) / 2, M = sigma0^2 * identity, every iteration weights
//   the whole stamp with the Gaussian of the current (r0, c0, M), w = exp(-1/2 d^T M^-1 d) * I, takes the weighted
//   centroid offset m and second moments C, and sets r0 += 2 m_r, c0 += 2 m_c, M = 2 C (a matched Gaussian is the fixed
//   point; the factor 2 undoes the narrowing of a Gaussian by a Gaussian weight).  Stops with status 0 when the step
//   2 max|m| and the relative change of M are below tol, 2 at max_iter, 3 when the moments degenerate (det M <= 1e-6, a
//   weighted flux that is not positive, a centroid that left the stamp, a negative or non-finite trace).
//
// One workgroup of 256 threads per stamp.  The stamp is read once: the chosen band plane goes to LDS as doubles
// (59^2 * 8 B = 27.8 KB) while the per-band flux and sigma^2 sums are taken; every iteration is then one pass over the LDS
// plane with six fp64 sums.  Reductions go butterfly within a wave, then through LDS in wave order (as posfit.hip): a
// stamp's result has the same bits wherever it sits in a batch.  Every thread runs the same scalar update on the reduced
// values: no divergence, no atomics.  fp64 VALU work; nothing here has a matrix shape for MFMA.  The reduction and the
// iteration itself are in measure_dev.h, which the PSF correction (regauss.hip) shares.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>
#include <cmath>

namespace dv {

namespace {
constexpr int MS_MAX_BANDS = 16;                  // the flux accumulators live in registers (the engine takes 1 .. 15 bands)
constexpr size_t MS_LDS_BUDGET = 64 * 1024;       // plane + reduction scratch; what a workgroup gets without opting in to more

// The measurement of one stamp by its workgroup: P / S the stamp's mean / stddev [cs][cs][nb] float32 (S null: no flux_err),
// the output pointers at the stamp's own rows.  ERR = false leaves the sigma^2 sums out altogether (the Monte-Carlo samples
// have no stddev stamp); the sums that remain are reduced in the same order, so the results have the same bits.
template <bool ERR>
__device__ __forceinline__ void measure_stamp(const float* __restrict__ P, const float* __restrict__ S, int cs, int nb,
                                              int band, double sigma0, double tol, int max_iter, double* __restrict__ flux,
                                              double* __restrict__ flux_err, double* __restrict__ sh,
                                              int* __restrict__ iters, int* __restrict__ status, double* s_mem) {
  const int npix = cs * cs;
  double* plane = s_mem;                    // [cs][cs]
  double* s_red = s_mem + npix;             // [MS_RED]

  // one pass over the stamp: the band plane to LDS, the per-band sums in registers
  double f[MS_MAX_BANDS], q[ERR ? MS_MAX_BANDS : 1];
#pragma unroll
  for (int b = 0; b < MS_MAX_BANDS; ++b) f[b] = 0.0;
#pragma unroll
  for (int b = 0; b < (ERR ? MS_MAX_BANDS : 1); ++b) q[b] = 0.0;
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
    const float* p = P + (long)e * nb;
    const float* sp = ERR && S ? S + (long)e * nb : nullptr;
#pragma unroll
    for (int b = 0; b < MS_MAX_BANDS; ++b) {
      if (b < nb) {
        const double v = (double)p[b];
        f[b] += v;
        if (b == band) plane[e] = v;
        if (ERR && sp) {
          const double sv = (double)sp[b];
          q[ERR ? b : 0] += sv * sv;
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < MS_MAX_BANDS; ++b) {
    if (b < nb) {                           // (nb is uniform: every thread takes the same barriers)
      if (ERR) {
        double a[2] = {f[b], q[ERR ? b : 0]};
        ms_block_sum<2>(a, s_red);
        if (threadIdx.x == 0) {
          flux[b] = a[0];
          if (flux_err) flux_err[b] = sqrt(a[1]);
        }
      } else {
        double a[1] = {f[b]};
        ms_block_sum<1>(a, s_red);
        if (threadIdx.x == 0) flux[b] = a[0];
      }
    }
  }
  // (every thread reads back only the plane elements it wrote itself: the loops above and below walk the same e)

  const double ctr = 0.5 * (double)(cs - 1);
  double r0 = ctr, c0 = ctr, Mrr = sigma0 * sigma0, Mrc = 0.0, Mcc = sigma0 * sigma0;
  int it = 0, st = 2;
  ms_iterate(plane, cs, tol, max_iter, r0, c0, Mrr, Mrc, Mcc, it, st, s_red);
  if (threadIdx.x == 0) {
    sh[0] = r0;
    sh[1] = c0;
    sh[2] = Mrr;
    sh[3] = Mrc;
    sh[4] = Mcc;
    *iters = it;
    *status = st;
  }
}

// mean / stddev: stamps [n][cs][cs][nb] float32 (stddev and flux_err null together); outputs indexed by stamp
__global__ __launch_bounds__(MS_THREADS) void measure_kernel(const float* __restrict__ mean, const float* __restrict__ stddev,
                                                             int cs, int nb, int band, double sigma0, double tol,
                                                             int max_iter, double* __restrict__ flux,
                                                             double* __restrict__ flux_err, double* __restrict__ shape,
                                                             int* __restrict__ iters, int* __restrict__ status) {
  extern __shared__ double s_mem[];
  const long gi = blockIdx.x;
  const long stamp = (long)cs * cs * nb;
  measure_stamp<true>(mean + gi * stamp, stddev ? stddev + gi * stamp : nullptr, cs, nb, band, sigma0, tol, max_iter,
                      flux + gi * nb, flux_err ? flux_err + gi * nb : nullptr, shape + gi * 5, iters + gi, status + gi, s_mem);
}

// ---- Monte-Carlo catalogue: every decode of every galaxy measured, the rows folded per galaxy ------------------
// One decoder pass as it lies in HBM: `rows` sample stamps [rows][cs][cs][nb], one workgroup each, measured without a stddev
// stamp into the pass's scratch rows.  The bits are measure_kernel's for the same stamp.
__global__ __launch_bounds__(MS_THREADS) void measure_mc_sample_kernel(const float* __restrict__ pass, int cs, int nb, int band,
                                                                       double sigma0, double tol, int max_iter,
                                                                       double* __restrict__ flux, double* __restrict__ shape,
                                                                       int* __restrict__ iters, int* __restrict__ status) {
  extern __shared__ double s_mem[];
  const long r = blockIdx.x;
  measure_stamp<false>(pass + r * cs * cs * nb, nullptr, cs, nb, band, sigma0, tol, max_iter, flux + r * nb, nullptr,
                       shape + r * 5, iters + r, status + r, s_mem);
}

// Welford's recurrence on one quantity, every operation rounded on its own
__device__ __forceinline__ void mc_fold(double x, double n, double& mean, double& m2) {
#pragma clang fp contract(off)
  const double d = x - mean;
  mean += d / n;
  m2 += d * (x - mean);
}

// Folds the scratch rows of one pass - row r * n + g is sample k0 + r of galaxy g of the pass's n galaxies - into the running
// state of those galaxies, in ascending sample order: (mean, M2) of the nb fluxes over all samples, (mean, M2) of the 8 shape
// quantities {row, col, Mrr, Mrc, Mcc, sigma, e1, e2} over the accepted samples (status 0, det > 0, tr > 0), counted in n_ok.
// The state lives in the output arrays themselves (M2 in the std arrays), whose pointers stand at the pass's first galaxy;
// k0 = 0 starts it, finish (the pass that holds sample S - 1) turns M2 into std = sqrt(M2 / n), NaN where n_ok = 0.  One
// thread per galaxy: a galaxy's result depends on nothing but its own samples; no atomics.
__global__ __launch_bounds__(256) void measure_mc_fold_kernel(const double* __restrict__ sflux, const double* __restrict__ sshape,
                                                              const int* __restrict__ sstatus, int n, int reps, int k0, int S,
                                                              int nb, int finish, double* __restrict__ fmean,
                                                              double* __restrict__ fstd, double* __restrict__ smean,
                                                              double* __restrict__ sstd, int* __restrict__ n_ok,
                                                              double* __restrict__ sample_flux,
                                                              double* __restrict__ sample_shape,
                                                              int* __restrict__ sample_status) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  for (int b = 0; b < nb; ++b) {
    double mean = k0 ? fmean[g * nb + b] : 0.0, m2 = k0 ? fstd[g * nb + b] : 0.0;
    for (int r = 0; r < reps; ++r) {
      const double x = sflux[((long)r * n + g) * nb + b];
      mc_fold(x, (double)(k0 + r + 1), mean, m2);
      if (sample_flux) sample_flux[(g * S + k0 + r) * nb + b] = x;
    }
    fmean[g * nb + b] = mean;
    fstd[g * nb + b] = finish ? __dsqrt_rn(m2 / (double)S) : m2;
  }
  double mean[8], m2[8];
  int cnt = k0 ? n_ok[g] : 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mean[k] = k0 ? smean[g * 8 + k] : 0.0;
    m2[k] = k0 ? sstd[g * 8 + k] : 0.0;
  }
  for (int r = 0; r < reps; ++r) {
    const long row = (long)r * n + g;
    double x[8];
#pragma unroll
    for (int k = 0; k < 5; ++k) x[k] = sshape[row * 5 + k];
    const int st = sstatus[row];
    if (sample_shape) {
#pragma unroll
      for (int k = 0; k < 5; ++k) sample_shape[(g * S + k0 + r) * 5 + k] = x[k];
      sample_status[g * S + k0 + r] = st;
    }
    const double Mrr = x[2], Mrc = x[3], Mcc = x[4];
    const double tr = Mcc + Mrr, det = Mrr * Mcc - Mrc * Mrc;
    if (st == 0 && det > 0.0 && tr > 0.0) {
      x[5] = __dsqrt_rn(__dsqrt_rn(det));
      x[6] = (Mcc - Mrr) / tr;
      x[7] = 2.0 * Mrc / tr;
      ++cnt;
#pragma unroll
      for (int k = 0; k < 8; ++k) mc_fold(x[k], (double)cnt, mean[k], m2[k]);
    }
  }
  n_ok[g] = cnt;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    smean[g * 8 + k] = finish && cnt == 0 ? nan : mean[k];
    sstd[g * 8 + k] = !finish ? m2[k] : cnt == 0 ? nan : __dsqrt_rn(m2[k] / (double)cnt);
  }
}
}  // namespace

size_t measure_lds_bytes(int cs) { return ((size_t)cs * cs + MS_RED) * sizeof(double); }

// the refusals of the measurement, before any GPU work
int measure_check(const char* who, int cs, int nb, int band, double sigma0, double tol, int max_iter) {
  if (cs < 1 || nb < 1 || nb > MS_MAX_BANDS) {
    set_error("%s: stamps of %d pixels and %d bands; the measurement takes 1 .. %d bands", who, cs, nb, MS_MAX_BANDS);
    return E_INVALID;
  }
  if (cs > 4096 || measure_lds_bytes(cs) > MS_LDS_BUDGET) {
    set_error("%s: the %d x %d band plane (%zu bytes as float64) does not fit the %zu bytes of LDS the measurement kernel "
              "uses: stamps of at most 90 pixels", who, cs, cs, (size_t)cs * cs * sizeof(double), MS_LDS_BUDGET);
    return E_INVALID;
  }
  if (band < 0 || band >= nb) {
    set_error("%s: band %d asked for, the stamps have bands 0 .. %d", who, band, nb - 1);
    return E_INVALID;
  }
  if (!(std::isfinite(sigma0) && sigma0 > 0.0) || !(std::isfinite(tol) && tol > 0.0)) {
    set_error("%s: sigma0 and tol must be finite and positive (got %g, %g)", who, sigma0, tol);
    return E_INVALID;
  }
  if (max_iter < 0) {
    set_error("%s: max_iter must be >= 0 (got %d)", who, max_iter);
    return E_INVALID;
  }
  return OK;
}

// n stamps that lie in device memory; every output pointer is the row of the first stamp (flux_err null with stddev)
int launch_measure(const float* mean_dev, const float* stddev_dev, int n, int cs, int nb, int band, double sigma0,
                   double tol, int max_iter, double* flux_dev, double* flux_err_dev, double* shape_dev, int* iters_dev,
                   int* status_dev, hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(measure_kernel, dim3((unsigned)n), dim3(MS_THREADS), measure_lds_bytes(cs), s, mean_dev,
                     flux_err_dev ? stddev_dev : nullptr, cs, nb, band, sigma0, tol, max_iter, flux_dev, flux_err_dev,
                     shape_dev, iters_dev, status_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

// the catalogue's columns; flux_err only with a stddev stamp
void catalogue_columns(Rows& r, CatRows& dev, const CatRows& host, int nb, bool err) {
  r.add(dev.flux, host.flux, nb);
  if (err) r.add(dev.flux_err, host.flux_err, nb);
  r.add(dev.shape, host.shape, 5);
  r.add(dev.iters, host.iters, 1);
  r.add(dev.status, host.status, 1);
}

// host stamps in, host catalogue out, a chunk of stamps at a time
int scene_measure(const float* mean_h, const float* stddev_h, int64_t N, int cs, int nb, int band, double sigma0, double tol,
                  int max_iter, const CatRows& o, hipStream_t s) {
  DV_TRY(measure_check("dv_scene_measure", cs, nb, band, sigma0, tol, max_iter));
  if (N < 0 || (N > 0 && (!mean_h || !o.flux || !o.shape || !o.iters || !o.status))) {
    set_error("dv_scene_measure: mean, flux, shape, iters and status must all be given");
    return E_INVALID;
  }
  if ((stddev_h == nullptr) != (o.flux_err == nullptr)) {
    set_error("dv_scene_measure: stddev and flux_err go together (both given or both null)");
    return E_INVALID;
  }
  const size_t stamp = (size_t)cs * cs * nb;
  float *mean = nullptr, *sd = nullptr;
  CatRows d{};
  Rows in, out;
  in.add(mean, mean_h, stamp);
  if (stddev_h) in.add(sd, stddev_h, stamp);
  catalogue_columns(out, d, o, nb, stddev_h != nullptr);
  return walk_rows(N, (int64_t)1 << 20, 0, in, out, s, [&](int64_t, int n) {
    return launch_measure(mean, sd, n, cs, nb, band, sigma0, tol, max_iter, d.flux, d.flux_err, d.shape, d.iters, d.status, s);
  });
}

// a decoder pass in device memory: `rows` sample stamps measured into the scratch rows
int launch_measure_mc_samples(const float* pass_dev, int rows, int cs, int nb, int band, double sigma0, double tol,
                              int max_iter, const McScratch& w, hipStream_t s) {
  if (rows <= 0) return OK;
  hipLaunchKernelGGL(measure_mc_sample_kernel, dim3((unsigned)rows), dim3(MS_THREADS), measure_lds_bytes(cs), s, pass_dev, cs,
                     nb, band, sigma0, tol, max_iter, w.flux, w.shape, w.iters, w.status);
  DV_HIP(hipGetLastError());
  return OK;
}

// the scratch rows of a pass of n galaxies x reps samples (the first is sample k0 of S) folded into rows row0 .. of the state
int launch_measure_mc_fold(const McScratch& w, int n, int reps, int k0, int S, int nb, const McState& st, int64_t row0,
                           hipStream_t s) {
  if (n <= 0 || reps <= 0) return OK;
  const size_t r = (size_t)row0;
  hipLaunchKernelGGL(measure_mc_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.flux, w.shape, w.status, n,
                     reps, k0, S, nb, k0 + reps == S ? 1 : 0, st.flux_mean + r * nb, st.flux_std + r * nb, st.shape_mean + r * 8,
                     st.shape_std + r * 8, st.n_ok + r, st.sample_flux ? st.sample_flux + r * S * nb : nullptr,
                     st.sample_shape ? st.sample_shape + r * S * 5 : nullptr,
                     st.sample_status ? st.sample_status + r * S : nullptr);
  DV_HIP(hipGetLastError());
  return OK;
}

// the Monte-Carlo catalogue's columns (the per-sample rows only when kept) and the scratch rows of a pass
void mc_columns(Rows& r, McState& dev, const McState& host, int nb, int S, bool keep) {
  r.add(dev.flux_mean, host.flux_mean, nb);
  r.add(dev.flux_std, host.flux_std, nb);
  r.add(dev.shape_mean, host.shape_mean, 8);
  r.add(dev.shape_std, host.shape_std, 8);
  r.add(dev.n_ok, host.n_ok, 1);
  if (!keep) return;
  r.add(dev.sample_flux, host.sample_flux, (size_t)S * nb);
  r.add(dev.sample_shape, host.sample_shape, (size_t)S * 5);
  r.add(dev.sample_status, host.sample_status, S);
}

void mc_scratch_columns(Rows& r, McScratch& dev, int nb, int reps) {
  r.add(dev.flux, nullptr, (size_t)reps * nb);
  r.add(dev.shape, nullptr, (size_t)reps * 5);
  r.add(dev.iters, nullptr, reps);
  r.add(dev.status, nullptr, reps);
}

// host sample stamps [S][N][cs][cs][nb] in, host Monte-Carlo catalogue out, in chunks of galaxies with all their samples: a
// chunk is one pass of n galaxies x S samples
int scene_measure_mc(const float* samples_h, int S, int64_t N, int cs, int nb, int band, double sigma0, double tol,
                     int max_iter, const McState& out_h, hipStream_t s) {
  const size_t stamp = (size_t)cs * cs * nb;
  float* pass = nullptr;
  McScratch w{};
  McState st{};
  Rows in, out;
  in.add(pass, nullptr, (size_t)S * stamp);            // (sample q of the chunk's n galaxies at q * n: copied below)
  mc_scratch_columns(out, w, nb, S);
  mc_columns(out, st, out_h, nb, S, out_h.sample_flux != nullptr);
  return walk_rows(N, ((int64_t)1 << 20) / S, 0, in, out, s, [&](int64_t base, int n) {
    for (int q = 0; q < S; ++q)
      DV_HIP(hipMemcpyAsync(pass + (size_t)q * n * stamp, samples_h + ((size_t)q * N + base) * stamp, (size_t)n * stamp * sizeof(float),
                            hipMemcpyHostToDevice, s));
    DV_TRY(launch_measure_mc_samples(pass, n * S, cs, nb, band, sigma0, tol, max_iter, w, s));
    return launch_measure_mc_fold(w, n, S, 0, S, nb, st, 0, s);
  });
}

}  // namespace dv
