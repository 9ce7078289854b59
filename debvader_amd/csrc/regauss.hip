// PSF-corrected shapes of deblended galaxies: the re-Gaussianization of Hirata & Seljak (2003), ending in a
// plain moment subtraction on the host.  The reference ships an empty debvader.measure package; the measurement is defined
// here.  float64 throughout.
//
// Per PSF Q [ps][ps] (regauss_psf_kernel, one workgroup of 256 threads each, once per call): the adaptive moments of Q by
// the iteration of measure.hip from the centre and psf_sigma0 -> (q0, M_P), iterations, status; FQ = sum Q;
// A_P = sum g_P Q / sum g_P^2 with g_P the Gaussian of (q0, M_P); the kurtosis psf_rho4; and the residual of the PSF against
// its own best Gaussian, eps[j] = (Q[j] - A_P g_P(j)) / FQ, which stays in device memory for the galaxy kernel.
//
// Per galaxy (regauss_kernel, one workgroup of 256 threads each): I = the band plane of its mean stamp, (r0, c0, M_I) and
// status its catalogue row (measure.hip), the PSF row psf_index picks.
//   status 4  the row is ineligible (status neither 0 nor 2, a value that is not finite, det M_I <= 1e-6)
//   status 5  psf_index outside 0 .. K - 1, or a PSF that is not usable (psf_status != 0, FQ not finite and positive,
//             det M_P <= 1e-6)
//   status 6  M_0 = M_I - M_P has Mrr <= 0 or det <= 1e-6: the galaxy is not resolved
//   (the six outputs of such a row are NaN, its iterations 0)
//   A_I = sum g_I I / sum g_I^2, F0 = 2 pi sqrt(det M_I) A_I, f0(d) = F0 / (2 pi sqrt(det M_0)) exp(-1/2 d^T M_0^-1 d)
//   I'(x) = I(x) - sum_j eps[j] f0(x - (r0, c0) - (j - q0)), j over the ps^2 PSF pixels in row-major order
//   the iteration of measure.hip on I' from (r0, c0, M_I) -> (r', c', M'), iterations, status 0 / 2 / 3
//   rho4 = sum e^(-rho^2 / 2) I' rho^4 / sum e^(-rho^2 / 2) I' at the final state (2 for a Gaussian)
//
// The convolution is the hot path: cs^2 ps^2 multiply-adds per galaxy (1.5 M at 59 / 21).  f0 depends on the integer
// difference x - j and one sub-pixel offset per galaxy, so its (cs + ps - 1)^2 values are tabulated once per galaxy: 6.2 k
// exp instead of 1.5 M.  The plane, eps and the table lie in dynamic LDS (81.5 KB at 59 / 21, 103 KB at 59 / 33: opted in
// above 64 KB).  A thread owns the pixels e = threadIdx.x + 256 k (at most 16: cs <= 64) and keeps their sums in registers;
// for every PSF pixel it reads eps[j] once (a broadcast) and one table value per owned pixel (consecutive threads read
// consecutive doubles but for the row breaks); the loop is compiled for every number of owned pixels, so those reads go
// out together (the LDS leaves room for one workgroup per CU: its latency is hidden within the wave).  A pixel's sum is taken by its one thread in ascending j, and the
// reductions go butterfly within the wave, then through LDS in wave order: a row has the same bits wherever it sits in a
// batch.  I' goes back over I in the plane - every thread writes the elements it owns, the ones the iteration has it read -
// and the iteration runs in place.  fp64 VALU; nothing here has a matrix shape for MFMA.  No atomics; thread 0 writes the
// row with ordinary stores.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>
#include <cmath>

namespace dv {

namespace {
constexpr int RG_MAX_CS = 64;                      // 16 owned pixels per thread
constexpr int RG_NPT = RG_MAX_CS * RG_MAX_CS / MS_THREADS;
constexpr int RG_MIN_PS = 5, RG_MAX_PS = 33;
constexpr size_t RG_LDS_MAX = 160 * 1024;          // what a gfx950 workgroup can be given

struct RgGauss { double r0, c0, qa, qb, qc; };

__device__ __forceinline__ RgGauss rg_gauss(double r0, double c0, double Mrr, double Mrc, double Mcc) {
  const double det = Mrr * Mcc - Mrc * Mrc;
  return RgGauss{r0, c0, -0.5 * Mcc / det, Mrc / det, -0.5 * Mrr / det};
}

__device__ __forceinline__ double rg_eval(const RgGauss& g, double dr, double dc) {
  return exp(g.qa * dr * dr + g.qb * dr * dc + g.qc * dc * dc);
}

// sum e^(-rho^2 / 2) v rho^4 / sum e^(-rho^2 / 2) v over plane [n][n] at the state (r0, c0, M); -1/2 rho^2 is the
// exponent of the Gaussian itself
__device__ __forceinline__ double rg_rho4(const double* plane, int n, const RgGauss& g, double* s_red) {
  double a[2] = {0.0, 0.0};
  for (int e = threadIdx.x; e < n * n; e += MS_THREADS) {
    const int r = e / n, c = e - r * n;
    const double dr = (double)r - g.r0, dc = (double)c - g.c0;
    const double h = g.qa * dr * dr + g.qb * dr * dc + g.qc * dc * dc;
    const double w = exp(h) * plane[e];
    a[0] += w;
    a[1] += w * (4.0 * h * h);
  }
  ms_block_sum<2>(a, s_red);
  return a[0] > 0.0 ? a[1] / a[0] : __longlong_as_double(0x7ff8000000000000LL);
}

// plane[e] -= sum_j eps[j] tab(x_e - j) for the NPT pixels e = threadIdx.x + k MS_THREADS a thread owns: pixel (r, c) and PSF
// pixel (jr, jc) meet at table entry (r - jr + ps - 1, c - jc + ps - 1).  NPT is a template argument so that the NPT table
// reads of one PSF pixel are issued together, ahead of the NPT multiply-adds that wait for them.
template <int NPT>
__device__ __forceinline__ void rg_convolve(double* plane, const double* s_eps, const double* s_tab, int cs, int ps) {
  static_assert(NPT >= 1 && NPT <= RG_NPT, "a thread owns at most RG_NPT pixels");
  const int npix = cs * cs, T = cs + ps - 1;
  int tb[NPT];
  double acc[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int e = min((int)threadIdx.x + k * MS_THREADS, npix - 1);   // (a thread without a k-th pixel repeats the last one and drops the sum)
    const int r = e / cs, c = e - r * cs;
    tb[k] = (r + ps - 1) * T + (c + ps - 1);
    acc[k] = 0.0;
  }
  for (int jr = 0; jr < ps; ++jr) {
    for (int jc = 0; jc < ps; ++jc) {
      const double ev = s_eps[jr * ps + jc];
      const int off = jr * T + jc;
#pragma unroll
      for (int k = 0; k < NPT; ++k) acc[k] += ev * s_tab[tb[k] - off];
    }
  }
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int e = (int)threadIdx.x + k * MS_THREADS;
    if (e < npix) plane[e] -= acc[k];
  }
}

// psf [K][ps][ps]; shape [K][5], aux [K][3] = {A_P, FQ, rho4}, iters [K], status [K], eps [K][ps][ps]
__global__ __launch_bounds__(MS_THREADS) void regauss_psf_kernel(const double* __restrict__ psf, int ps, double sigma0,
                                                                 double tol, int max_iter, double* __restrict__ shape,
                                                                 double* __restrict__ aux, int* __restrict__ iters,
                                                                 int* __restrict__ status, double* __restrict__ eps) {
  extern __shared__ double s_mem[];
  const int npix = ps * ps;
  double* plane = s_mem;                    // [ps][ps]
  double* s_red = s_mem + npix;             // [MS_RED]
  const long k = blockIdx.x;
  const double* Q = psf + k * npix;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double f[1] = {0.0};
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
    const double v = Q[e];
    plane[e] = v;
    f[0] += v;
  }
  ms_block_sum<1>(f, s_red);
  const double FQ = f[0];
  const double ctr = 0.5 * (double)(ps - 1);
  double r0 = ctr, c0 = ctr, Mrr = sigma0 * sigma0, Mrc = 0.0, Mcc = sigma0 * sigma0;
  int it = 0, st = 2;
  ms_iterate(plane, ps, tol, max_iter, r0, c0, Mrr, Mrc, Mcc, it, st, s_red);
  const double det = Mrr * Mcc - Mrc * Mrc;
  const bool ok = st != 3 && ms_finite(det) && det > 1e-6;   // (uniform: every thread holds the same state)
  double AP = nan, rho4 = nan;
  if (ok) {
    const RgGauss g = rg_gauss(r0, c0, Mrr, Mrc, Mcc);
    double a[2] = {0.0, 0.0};
    for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
      const int r = e / ps, c = e - r * ps;
      const double w = rg_eval(g, (double)r - r0, (double)c - c0);
      a[0] += w * plane[e];
      a[1] += w * w;
    }
    ms_block_sum<2>(a, s_red);
    AP = a[0] / a[1];
    rho4 = rg_rho4(plane, ps, g, s_red);
    for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
      const int r = e / ps, c = e - r * ps;
      eps[k * npix + e] = (plane[e] - AP * rg_eval(g, (double)r - r0, (double)c - c0)) / FQ;
    }
  } else {
    for (int e = threadIdx.x; e < npix; e += MS_THREADS) eps[k * npix + e] = nan;   // (no galaxy reads it: the PSF is not usable)
  }
  if (threadIdx.x == 0) {
    shape[k * 5 + 0] = r0;
    shape[k * 5 + 1] = c0;
    shape[k * 5 + 2] = Mrr;
    shape[k * 5 + 3] = Mrc;
    shape[k * 5 + 4] = Mcc;
    aux[k * 3 + 0] = AP;
    aux[k * 3 + 1] = FQ;
    aux[k * 3 + 2] = rho4;
    iters[k] = it;
    status[k] = st;
  }
}

// stamps [n][cs][cs][nb] float32; shape [n][5], status [n], psf_index [n]: the rows of the n stamps; the PSF rows and eps of
// regauss_psf_kernel; out [n][6] = {r', c', Mrr', Mrc', Mcc', rho4}, out_iters [n], out_status [n]
__global__ __launch_bounds__(MS_THREADS) void regauss_kernel(const float* __restrict__ stamps, const double* __restrict__ shape,
                                                             const int* __restrict__ status,
                                                             const int* __restrict__ psf_index, int cs, int nb, int band,
                                                             const double* __restrict__ psf_shape,
                                                             const double* __restrict__ psf_aux,
                                                             const int* __restrict__ psf_status,
                                                             const double* __restrict__ psf_eps, int K, int ps, double tol,
                                                             int max_iter, double* __restrict__ out,
                                                             int* __restrict__ out_iters, int* __restrict__ out_status) {
  extern __shared__ double s_mem[];
  const int npix = cs * cs, npsf = ps * ps, T = cs + ps - 1;
  double* plane = s_mem;                    // [cs][cs]: I, then I'
  double* s_eps = plane + npix;             // [ps][ps]
  double* s_tab = s_eps + npsf;             // [T][T]: f0 at the integer differences x - j = -(ps - 1) .. cs - 1
  double* s_red = s_tab + T * T;            // [MS_RED]
  const long gi = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // eligibility: the same answer in every thread (all read the same rows)
  const double* sh = shape + gi * 5;
  double r0 = sh[0], c0 = sh[1], Mrr = sh[2], Mrc = sh[3], Mcc = sh[4];
  const int st_in = status[gi], pi = psf_index[gi];
  const double detI = Mrr * Mcc - Mrc * Mrc;
  int fail = 0;
  double q0r = 0.0, q0c = 0.0, Zrr = 0.0, Zrc = 0.0, Zcc = 0.0, det0 = 0.0;
  if ((st_in != 0 && st_in != 2) || !(ms_finite(r0) && ms_finite(c0) && ms_finite(Mrr) && ms_finite(Mrc) && ms_finite(Mcc)) ||
      !(ms_finite(detI) && detI > 1e-6)) {
    fail = 4;
  } else if (pi < 0 || pi >= K) {
    fail = 5;
  } else {
    const double* p = psf_shape + (long)pi * 5;
    const double Prr = p[2], Prc = p[3], Pcc = p[4], FQ = psf_aux[(long)pi * 3 + 1];
    const double detP = Prr * Pcc - Prc * Prc;
    if (psf_status[pi] != 0 || !(ms_finite(FQ) && FQ > 0.0) || !(ms_finite(detP) && detP > 1e-6)) {
      fail = 5;
    } else {
      q0r = p[0];
      q0c = p[1];
      Zrr = Mrr - Prr;
      Zrc = Mrc - Prc;
      Zcc = Mcc - Pcc;
      det0 = Zrr * Zcc - Zrc * Zrc;
      if (!(Zrr > 0.0) || !(ms_finite(det0) && det0 > 1e-6)) fail = 6;
    }
  }
  if (fail) {
    if (threadIdx.x == 0) {
      for (int k = 0; k < 6; ++k) out[gi * 6 + k] = nan;
      out_iters[gi] = 0;
      out_status[gi] = fail;
    }
    return;
  }

  // the band plane and the PSF's residual to LDS; A_I under the galaxy's own weight
  const RgGauss gI = rg_gauss(r0, c0, Mrr, Mrc, Mcc);
  const float* P = stamps + gi * npix * nb + band;
  double a[2] = {0.0, 0.0};
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
    const int r = e / cs, c = e - r * cs;
    const double v = (double)P[(long)e * nb];
    plane[e] = v;
    const double w = rg_eval(gI, (double)r - r0, (double)c - c0);
    a[0] += w * v;
    a[1] += w * w;
  }
  for (int e = threadIdx.x; e < npsf; e += MS_THREADS) s_eps[e] = psf_eps[(long)pi * npsf + e];
  ms_block_sum<2>(a, s_red);
  const double two_pi = 6.283185307179586476925286766559;
  const double F0 = two_pi * sqrt(detI) * (a[0] / a[1]);
  const double amp = F0 / (two_pi * sqrt(det0));

  // the table of f0: entry (u, v) holds f0((u - (ps - 1)) - (r0 - q0r), (v - (ps - 1)) - (c0 - q0c))
  const RgGauss g0 = rg_gauss(0.0, 0.0, Zrr, Zrc, Zcc);
  const double offr = (double)(ps - 1) + (r0 - q0r), offc = (double)(ps - 1) + (c0 - q0c);
  for (int e = threadIdx.x; e < T * T; e += MS_THREADS) {
    const int u = e / T, v = e - u * T;
    s_tab[e] = amp * rg_eval(g0, (double)u - offr, (double)v - offc);
  }
  __syncthreads();                          // eps and the table are complete

  // the convolution, for the number of pixels a thread owns: <= RG_NPT (regauss_check)
  switch ((npix + MS_THREADS - 1) / MS_THREADS) {
#define RG_CASE(n) case n: rg_convolve<n>(plane, s_eps, s_tab, cs, ps); break;
    RG_CASE(1) RG_CASE(2) RG_CASE(3) RG_CASE(4) RG_CASE(5) RG_CASE(6) RG_CASE(7) RG_CASE(8)
    RG_CASE(9) RG_CASE(10) RG_CASE(11) RG_CASE(12) RG_CASE(13) RG_CASE(14) RG_CASE(15) RG_CASE(16)
#undef RG_CASE
  }

  // the moments of I', from the galaxy's own row
  int it = 0, st = 2;
  ms_iterate(plane, cs, tol, max_iter, r0, c0, Mrr, Mrc, Mcc, it, st, s_red);
  double rho4 = nan;
  if (st != 3) rho4 = rg_rho4(plane, cs, rg_gauss(r0, c0, Mrr, Mrc, Mcc), s_red);   // (uniform)
  if (threadIdx.x == 0) {
    out[gi * 6 + 0] = r0;
    out[gi * 6 + 1] = c0;
    out[gi * 6 + 2] = Mrr;
    out[gi * 6 + 3] = Mrc;
    out[gi * 6 + 4] = Mcc;
    out[gi * 6 + 5] = rho4;
    out_iters[gi] = it;
    out_status[gi] = st;
  }
}

size_t regauss_psf_lds_bytes(int ps) { return ((size_t)ps * ps + MS_RED) * sizeof(double); }
}  // namespace

size_t regauss_lds_bytes(int cs, int ps) {
  const size_t T = (size_t)cs + ps - 1;
  return ((size_t)cs * cs + (size_t)ps * ps + T * T + MS_RED) * sizeof(double);
}

// the refusals of the correction, before any GPU work
int regauss_check(const char* who, int cs, int nb, int band, int K, int ps, double psf_sigma0, double tol, int max_iter) {
  if (cs < 1 || cs > RG_MAX_CS || nb < 1 || nb > 4096) {
    set_error("%s: stamps of %d pixels and %d bands; the PSF correction takes 1 .. %d pixels and 1 .. 4096 bands", who, cs, nb,
              RG_MAX_CS);
    return E_INVALID;
  }
  if (band < 0 || band >= nb) {
    set_error("%s: band %d asked for, the stamps have bands 0 .. %d", who, band, nb - 1);
    return E_INVALID;
  }
  if (K < 1) {
    set_error("%s: %d PSF images given, at least 1 is needed", who, K);
    return E_INVALID;
  }
  if (ps < RG_MIN_PS || ps > RG_MAX_PS) {
    set_error("%s: PSF images of %d pixels; %d .. %d are taken", who, ps, RG_MIN_PS, RG_MAX_PS);
    return E_INVALID;
  }
  if (regauss_lds_bytes(cs, ps) > RG_LDS_MAX) {
    set_error("%s: a %d-pixel stamp with a %d-pixel PSF needs %zu bytes of LDS (plane, PSF residual and the table of the "
              "model galaxy), a workgroup has %zu", who, cs, ps, regauss_lds_bytes(cs, ps), RG_LDS_MAX);
    return E_INVALID;
  }
  if (!(std::isfinite(psf_sigma0) && psf_sigma0 > 0.0) || !(std::isfinite(tol) && tol > 0.0)) {
    set_error("%s: psf_sigma0 and tol must be finite and positive (got %g, %g)", who, psf_sigma0, tol);
    return E_INVALID;
  }
  if (max_iter < 0) {
    set_error("%s: max_iter must be >= 0 (got %d)", who, max_iter);
    return E_INVALID;
  }
  return OK;
}

int RegaussPsf::alloc(int K, int ps) {
  DV_TRY(img.alloc((size_t)K * ps * ps));
  DV_TRY(eps.alloc((size_t)K * ps * ps));
  DV_TRY(shape.alloc((size_t)K * 5));
  DV_TRY(aux.alloc((size_t)K * 3));
  DV_TRY(iters.alloc((size_t)K));
  return status.alloc((size_t)K);
}

// the K PSF images uploaded and measured on stream s
int RegaussPsf::measure(const double* psf_h, int K, int ps, double psf_sigma0, double tol, int max_iter, hipStream_t s) {
  DV_HIP(hipMemcpyAsync(img, psf_h, (size_t)K * ps * ps * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(regauss_psf_kernel, dim3((unsigned)K), dim3(MS_THREADS), regauss_psf_lds_bytes(ps), s, img.get(), ps,
                     psf_sigma0, tol, max_iter, shape.get(), aux.get(), iters.get(), status.get(), eps.get());
  DV_HIP(hipGetLastError());
  return OK;
}

int RegaussPsf::download(int K, double* shape_h, double* aux_h, int32_t* iters_h, int32_t* status_h, hipStream_t s) {
  DV_HIP(hipMemcpyAsync(shape_h, shape, (size_t)K * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(aux_h, aux, (size_t)K * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(iters_h, iters, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(status_h, status, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, s));
  return OK;
}

// n stamps that lie in device memory; every per-galaxy pointer is the row of the first stamp
int launch_regauss(const float* stamps_dev, const double* shape_dev, const int* status_dev, const int* psf_index_dev, int n,
                   int cs, int nb, int band, const RegaussPsf& psf, int K, int ps, double tol, int max_iter, double* out_dev,
                   int* iters_dev, int* ostatus_dev, hipStream_t s) {
  if (n <= 0) return OK;
  const size_t smem = regauss_lds_bytes(cs, ps);
  static size_t attr_bytes = 64 * 1024;     // what a workgroup gets without opting in to more
  if (smem > attr_bytes) {
    DV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(regauss_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)RG_LDS_MAX));
    attr_bytes = RG_LDS_MAX;
  }
  hipLaunchKernelGGL(regauss_kernel, dim3((unsigned)n), dim3(MS_THREADS), smem, s, stamps_dev, shape_dev, status_dev,
                     psf_index_dev, cs, nb, band, psf.shape.get(), psf.aux.get(), psf.status.get(), psf.eps.get(), K, ps, tol,
                     max_iter, out_dev, iters_dev, ostatus_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

void regauss_columns(Rows& r, RegaussRows& dev, const RegaussRows& host) {
  r.add(dev.out, host.out, 6);
  r.add(dev.iters, host.iters, 1);
  r.add(dev.status, host.status, 1);
}

// host arrays in, host rows out, a chunk of stamps at a time (half of free device memory less the PSFs); the PSFs are
// uploaded and measured once
int scene_regauss(const float* stamps_h, const double* shape_h, const int32_t* status_h, const int32_t* psf_index_h, int64_t N,
                  int cs, int nb, int band, const double* psf_h, int K, int ps, double psf_sigma0, double tol, int max_iter,
                  const RegaussRows& out_h, double* psf_shape_h, double* psf_aux_h, int32_t* psf_iters_h,
                  int32_t* psf_status_h, hipStream_t s) {
  const char* who = "dv_scene_regauss";
  DV_TRY(regauss_check(who, cs, nb, band, K, ps, psf_sigma0, tol, max_iter));
  if (!psf_h || !psf_shape_h || !psf_aux_h || !psf_iters_h || !psf_status_h) {
    set_error("%s: psf, psf_shape, psf_aux, psf_iters and psf_status must all be given", who);
    return E_INVALID;
  }
  if (N < 0 || (N > 0 && (!stamps_h || !shape_h || !status_h || !psf_index_h || !out_h.out || !out_h.iters || !out_h.status))) {
    set_error("%s: stamps, shape, status, psf_index, regauss, regauss_iters and regauss_status must all be given", who);
    return E_INVALID;
  }
  RegaussPsf psf;
  DV_TRY(psf.alloc(K, ps));
  StreamDrain drain(s);
  DV_TRY(psf.measure(psf_h, K, ps, psf_sigma0, tol, max_iter, s));
  DV_TRY(psf.download(K, psf_shape_h, psf_aux_h, psf_iters_h, psf_status_h, s));
  DV_HIP(hipStreamSynchronize(s));
  float* stamps = nullptr;
  double* shape = nullptr;
  int *status = nullptr, *index = nullptr;
  RegaussRows d{};
  Rows in, out;
  in.add(stamps, stamps_h, (size_t)cs * cs * nb);
  in.add(shape, shape_h, 5);
  in.add(status, status_h, 1);
  in.add(index, psf_index_h, 1);
  regauss_columns(out, d, out_h);
  drain.dismiss();                                     // (the stream is idle; from here on the walker waits)
  return walk_rows(N, (int64_t)1 << 20, RegaussPsf::bytes(K, ps), in, out, s, [&](int64_t, int n) {
    return launch_regauss(stamps, shape, status, index, n, cs, nb, band, psf, K, ps, tol, max_iter, d.out, d.iters, d.status, s);
  });
}

}  // namespace dv
