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
// values: no divergence, no atomics.  fp64 VALU work; nothing here has a matrix shape for MFMA.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace dv {

namespace {
constexpr int MS_THREADS = 256;
constexpr int MS_MAX_BANDS = 16;                  // the flux accumulators live in registers (the engine takes 1 .. 15 bands)
constexpr size_t MS_LDS_BUDGET = 64 * 1024;       // plane + reduction scratch; what a workgroup gets without opting in to more
constexpr int MS_RED = 4 * 6;                     // reduction scratch, doubles

// sum of v over the workgroup, the same order on every call; every thread gets the result
template <int K>
__device__ __forceinline__ void ms_block_sum(double (&v)[K], double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  __syncthreads();                          // s_red of the previous call has been read by everyone
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((s_red[k] + s_red[K + k]) + (s_red[2 * K + k] + s_red[3 * K + k]));
}

__device__ __forceinline__ bool ms_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

// mean / stddev: stamps [n][cs][cs][nb] float32 (stddev and flux_err null together); outputs indexed by stamp
__global__ __launch_bounds__(MS_THREADS) void measure_kernel(const float* __restrict__ mean, const float* __restrict__ stddev,
                                                             int cs, int nb, int band, double sigma0, double tol,
                                                             int max_iter, double* __restrict__ flux,
                                                             double* __restrict__ flux_err, double* __restrict__ shape,
                                                             int* __restrict__ iters, int* __restrict__ status) {
  extern __shared__ double s_mem[];
  const int npix = cs * cs;
  double* plane = s_mem;                    // [cs][cs]
  double* s_red = s_mem + npix;             // [MS_RED]
  const long gi = blockIdx.x;
  const float* P = mean + gi * npix * nb;
  const float* S = stddev ? stddev + gi * npix * nb : nullptr;

  // one pass over the stamp: the band plane to LDS, the per-band sums in registers
  double f[MS_MAX_BANDS], q[MS_MAX_BANDS];
#pragma unroll
  for (int b = 0; b < MS_MAX_BANDS; ++b) f[b] = q[b] = 0.0;
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
    const float* p = P + (long)e * nb;
    const float* sp = S ? S + (long)e * nb : nullptr;
#pragma unroll
    for (int b = 0; b < MS_MAX_BANDS; ++b) {
      if (b < nb) {
        const double v = (double)p[b];
        f[b] += v;
        if (b == band) plane[e] = v;
        if (sp) {
          const double sv = (double)sp[b];
          q[b] += sv * sv;
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < MS_MAX_BANDS; ++b) {
    if (b < nb) {                           // (nb is uniform: every thread takes the same barriers)
      double a[2] = {f[b], q[b]};
      ms_block_sum<2>(a, s_red);
      if (threadIdx.x == 0) {
        flux[gi * nb + b] = a[0];
        if (flux_err) flux_err[gi * nb + b] = sqrt(a[1]);
      }
    }
  }
  // (every thread reads back only the plane elements it wrote itself: the loops above and below walk the same e)

  const double ctr = 0.5 * (double)(cs - 1), half = 0.5 * (double)cs;
  double r0 = ctr, c0 = ctr, Mrr = sigma0 * sigma0, Mrc = 0.0, Mcc = sigma0 * sigma0;
  int it = 0, st = 2;
  const int step_r = MS_THREADS / cs, step_c = MS_THREADS - step_r * cs;
  for (int k = 1; k <= max_iter; ++k) {
    it = k;
    const double det = Mrr * Mcc - Mrc * Mrc;
    if (!(ms_finite(det) && det > 1e-6)) { st = 3; break; }
    // -1/2 (Mcc dr^2 - 2 Mrc dr dc + Mrr dc^2) / det = qa dr^2 + qb dr dc + qc dc^2
    const double qa = -0.5 * Mcc / det, qb = Mrc / det, qc = -0.5 * Mrr / det;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // w, w dr, w dc, w dr^2, w dr dc, w dc^2
    int pr = threadIdx.x / cs, pc = threadIdx.x - pr * cs;
    for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
      const double dr = (double)pr - r0, dc = (double)pc - c0;
      const double w = exp(qa * dr * dr + qb * dr * dc + qc * dc * dc) * plane[e];
      const double wr = w * dr, wc = w * dc;
      a[0] += w;
      a[1] += wr;
      a[2] += wc;
      a[3] += wr * dr;
      a[4] += wr * dc;
      a[5] += wc * dc;
      pc += step_c;
      pr += step_r;
      if (pc >= cs) { pc -= cs; ++pr; }
    }
    ms_block_sum<6>(a, s_red);
    const double S0 = a[0];
    if (!(ms_finite(S0) && S0 > 0.0)) { st = 3; break; }
    const double mr = a[1] / S0, mc = a[2] / S0;
    const double Nrr = 2.0 * (a[3] / S0 - mr * mr), Nrc = 2.0 * (a[4] / S0 - mr * mc), Ncc = 2.0 * (a[5] / S0 - mc * mc);
    const double step = 2.0 * fmax(fabs(mr), fabs(mc));
    const double tr = Nrr + Ncc;
    const double dM = fmax(fmax(fabs(Nrr - Mrr), fabs(Nrc - Mrc)), fabs(Ncc - Mcc)) / tr;
    r0 += 2.0 * mr;
    c0 += 2.0 * mc;
    Mrr = Nrr;
    Mrc = Nrc;
    Mcc = Ncc;
    // (a zero trace goes on: the next iteration's determinant test ends it)
    if (!(fabs(r0 - ctr) <= half) || !(fabs(c0 - ctr) <= half) || !(ms_finite(tr) && tr >= 0.0)) { st = 3; break; }
    if (step < tol && dM < tol) { st = 0; break; }
  }
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

// host stamps in, host catalogue out, in chunks of at most `chunk` stamps (sized by the caller against free device memory)
int scene_measure(const float* mean_h, const float* stddev_h, int64_t N, int cs, int nb, int band, double sigma0, double tol,
                  int max_iter, double* flux_h, double* flux_err_h, double* shape_h, int32_t* iters_h, int32_t* status_h,
                  int64_t chunk, hipStream_t s) {
  DV_TRY(measure_check("dv_scene_measure", cs, nb, band, sigma0, tol, max_iter));
  if (N < 0 || (N > 0 && (!mean_h || !flux_h || !shape_h || !iters_h || !status_h))) {
    set_error("dv_scene_measure: mean, flux, shape, iters and status must all be given");
    return E_INVALID;
  }
  if ((stddev_h == nullptr) != (flux_err_h == nullptr)) {
    set_error("dv_scene_measure: stddev and flux_err go together (both given or both null)");
    return E_INVALID;
  }
  if (N == 0) return OK;
  const size_t stamp = (size_t)cs * cs * nb;
  chunk = std::max<int64_t>(1, std::min<int64_t>({chunk, N, (int64_t)1 << 20}));
  DevBuf<float> mean, sd;
  DevBuf<double> flux, ferr, shape;
  DevBuf<int> it, st;
  DV_TRY(mean.alloc((size_t)chunk * stamp));
  if (stddev_h) {
    DV_TRY(sd.alloc((size_t)chunk * stamp));
    DV_TRY(ferr.alloc((size_t)chunk * nb));
  }
  DV_TRY(flux.alloc((size_t)chunk * nb));
  DV_TRY(shape.alloc((size_t)chunk * 5));
  DV_TRY(it.alloc((size_t)chunk));
  DV_TRY(st.alloc((size_t)chunk));
  for (int64_t base = 0; base < N; base += chunk) {
    const int n = (int)std::min<int64_t>(chunk, N - base);
    DV_HIP(hipMemcpyAsync(mean, mean_h + (size_t)base * stamp, (size_t)n * stamp * sizeof(float), hipMemcpyHostToDevice, s));
    if (sd)
      DV_HIP(hipMemcpyAsync(sd, stddev_h + (size_t)base * stamp, (size_t)n * stamp * sizeof(float), hipMemcpyHostToDevice, s));
    DV_TRY(launch_measure(mean, sd, n, cs, nb, band, sigma0, tol, max_iter, flux, ferr, shape, it, st, s));
    DV_HIP(hipMemcpyAsync(flux_h + (size_t)base * nb, flux, (size_t)n * nb * sizeof(double), hipMemcpyDeviceToHost, s));
    if (ferr)
      DV_HIP(hipMemcpyAsync(flux_err_h + (size_t)base * nb, ferr, (size_t)n * nb * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(shape_h + (size_t)base * 5, shape, (size_t)n * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(iters_h + base, it, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(status_h + base, st, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipStreamSynchronize(s));               // the device buffers are reused by the next chunk
  }
  return OK;
}

}  // namespace dv
