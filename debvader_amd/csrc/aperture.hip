// Aperture photometry of deblended galaxies: fluxes in fixed circular apertures, the Kron radius, the flux in
// the automatic (Kron) ellipse and the radii that hold given fractions of it.  The reference ships an empty debvader.measure
// package; the measurement is defined here.  float64 throughout.
//
// Per galaxy: P its mean stamp [cs][cs][nb] and S its stddev stamp (float32 widened; S may be absent), {r0, c0, Mrr, Mrc,
// Mcc} and status its catalogue row (measure.hip), I = P[:, :, band].  Eligible as in blend.hip: status 0 or 2, five finite
// shape values, det = Mrr Mcc - Mrc^2 finite and above 1e-6; otherwise aper_status 4, every float output NaN, flags 0.
//   q(x, y) = (a x) x + (b x) y + (c y) y,   a = Mcc / det, b = (-2 Mrc) / det, c = Mrr / det   (a circle: a = c = 1, b = 0)
//   weight of pixel (r, c) in the region q <= rho^2: the share of its s x s sub-pixel centres (dr + o_i, dc + o_j),
//   o_i = (i + 0.5) / s - 0.5, that lie inside: w = n / s^2, carried as the count n - a sum of w x is taken as the sum of n x
//   over s^2, one division per sum, and the sum of the weights themselves adds whole numbers, exact in any order.  A pixel
//   whose centre decides all of its sub-pixels is not counted: with
//   qc = sqrt(q(dr, dc)) and m = 0.7072 sqrt(a + c) it is wholly inside if qc + m <= rho, wholly outside if qc - m >= rho
//   (sqrt q is a norm and 0.7072 > sqrt(1/2), so the shortcut cannot change a count).  Sums run over the pixels of weight > 0.
//   1. circle k, every band:   ap_flux = sum w P, ap_flux_err = sqrt(sum w S^2), ap_area = sum w
//   2. Kron radius, at band:   r1 = sum sqrt(q) I / sum I over the pixel centres with q <= kron_limit^2; sum I not finite or
//                              not positive, or r1 not finite: aper_status 7, items 2 - 4 NaN
//                              rho_auto = kron_factor r1, or kron_min where that is smaller (flag bit 10)
//   3. the ellipse rho_auto, every band: flux_auto, flux_auto_err, auto_area
//   4. flux radii, at band:    F(rho) = sum w_rho I; bisect_iters halvings of [0, rho_auto] towards F = f_j flux_auto[band],
//                              the upper end is flux_rho[j] (in units of the moment ellipse)
//
// One workgroup of 256 threads per galaxy (aperture_kernel, ERR = false without a stddev stamp).  The band plane lies in
// dynamic LDS as doubles beside the reduction scratch, the sub-pixel offsets and the radii and fractions: 8 cs^2 + 384 bytes,
// within 64 KB up to cs = 90.  The Kron pass and the J x bisect_iters passes of the bisection run on that plane; the K + 1
// all-band passes read the float32 stamps from global memory, and only where the weight is positive, with 16 statically
// indexed band slots for the flux and 16 for the variance as measure.hip keeps them, one aperture per pass.  The s^2
// sub-pixel tests of a boundary pixel are a loop without early exit.  A pass visits only the box of the stamp its region can
// reach (ApWalk): about 20 x 20 pixels for a 2.5-px galaxy in a 59-px stamp, a ninth of the stamp.  Floating-point
// contraction is off in this file, every expression is evaluated left to right with only + - * / and the correctly rounded
// square root: a float64 restatement of the same scalar operations takes every inside / outside decision with the same bits.
// Reductions go butterfly within the
// wave, then through LDS in wave order (measure_dev.h): a row has the same bits wherever it sits in a batch.  Every thread
// holds the same reduced values, so the bisection branches uniformly.  fp64 VALU; nothing here has a matrix shape for MFMA.
// No atomics; thread 0 writes the rows with ordinary stores.
//
// The same apertures on the observed field with the neighbours subtracted: sum w (D - T + P) splits into the
// child sum above and the sums of w T and w D over the stamp pixels inside the field, T the completed mean field and D the
// observed field.  aperture_field_kernel takes the two field sums and the area inside the field for the K circles and the
// automatic ellipse (rho_auto read from the galaxy's aperture row): one workgroup per galaxy, K + 1 passes with the walk, the
// count and the reduction of ap_all_bands, nb contiguous doubles of T and of D per pixel of positive count, 16 + 16 statically
// indexed band slots, no plane - 352 bytes of static LDS.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#pragma clang fp contract(off)

namespace dv {

namespace {
constexpr int AP_MAX_BANDS = 16;                   // as measure.hip: the flux accumulators live in registers
constexpr int AP_SCRATCH = MS_RED + 12 + AP_MAX_RADII + AP_MAX_FRACTIONS;   // reduction, offsets (9, padded), radii, fractions
constexpr size_t AP_LDS_BUDGET = 64 * 1024;

// q = (a x) x + (b x) y + (c y) y, m the margin of the centre test, (er, ec) the half-extents in r and c of the region
// q <= 1 (NaN where the form is not positive definite: no extent is known)
struct ApForm { double a, b, c, m, er, ec; };

__device__ __forceinline__ ApForm ap_form(double a, double b, double c, double er, double ec) {
  return ApForm{a, b, c, 0.7072 * __dsqrt_rn(a + c), er, ec};
}

__device__ __forceinline__ double ap_q(const ApForm& f, double x, double y) { return (f.a * x) * x + (f.b * x) * y + (f.c * y) * y; }

// how many of the s x s sub-pixel centres of the pixel whose centre lies at (dr, dc) from the galaxy's are in the region
// q <= rho^2
__device__ __forceinline__ int ap_count(const ApForm& f, double rho, double dr, double dc, int s, const double* s_off) {
  const double qc = __dsqrt_rn(ap_q(f, dr, dc));
  if (qc + f.m <= rho) return s * s;
  if (qc - f.m >= rho) return 0;
  const double rho2 = rho * rho;
  int cnt = 0;
  for (int i = 0; i < s; ++i) {
    const double x = dr + s_off[i];
    for (int j = 0; j < s; ++j) cnt += ap_q(f, x, dc + s_off[j]) <= rho2 ? 1 : 0;
  }
  return cnt;
}

// The pixels a pass visits: the box of the stamp outside which no sub-pixel can lie in the region q <= rho^2 - its extent
// about (r0, c0) plus half a pixel for the sub-pixel offsets and one pixel for the rounding of the extent itself; the whole
// stamp where no extent is known.  A pixel outside the region counts 0 and is in no sum, so the box leaves every sum's terms
// alone.  A thread walks the box pixels i = threadIdx.x + k MS_THREADS in row-major order without a division per pixel.
struct ApWalk {
  int r_lo, c_lo, w, n, pr, pc, step_r, step_c;
  __device__ __forceinline__ ApWalk(int cs, const ApForm& f, double rho, double r0, double c0) {
    const double hr = rho * f.er + 1.5, hc = rho * f.ec + 1.5, top = (double)(cs - 1);
    // (fmax / fmin return the other operand for a NaN: the whole stamp)
    const int r_hi = (int)fmax(-1.0, fmin(top, ceil(r0 + hr))), c_hi = (int)fmax(-1.0, fmin(top, ceil(c0 + hc)));
    r_lo = (int)fmin(top + 1.0, fmax(0.0, floor(r0 - hr)));
    c_lo = (int)fmin(top + 1.0, fmax(0.0, floor(c0 - hc)));
    w = max(c_hi - c_lo + 1, 0);
    n = w * max(r_hi - r_lo + 1, 0);
    const int wd = max(w, 1);
    step_r = MS_THREADS / wd;
    step_c = MS_THREADS - step_r * wd;
    pr = (int)threadIdx.x / wd;
    pc = (int)threadIdx.x - pr * wd;
  }
  __device__ __forceinline__ int row() const { return r_lo + pr; }
  __device__ __forceinline__ int col() const { return c_lo + pc; }
  __device__ __forceinline__ void next() {
    pc += step_c;
    pr += step_r;
    if (pc >= w) { pc -= w; ++pr; }
  }
};

// F(rho) on the band plane
__device__ __forceinline__ double ap_plane_flux(const double* plane, int cs, const ApForm& f, double rho, double r0, double c0,
                                                int s, const double* s_off, double* s_red) {
  double a[1] = {0.0};
  ApWalk p(cs, f, rho, r0, c0);
  for (int i = threadIdx.x; i < p.n; i += MS_THREADS, p.next()) {
    const int cnt = ap_count(f, rho, (double)p.row() - r0, (double)p.col() - c0, s, s_off);
    if (cnt > 0) a[0] += (double)cnt * plane[p.row() * cs + p.col()];
  }
  ms_block_sum<1>(a, s_red);
  return a[0] / (double)(s * s);
}

// One aperture in every band: flux [nb], err [nb] (ERR), *area by thread 0; returns the flux of `band` in every thread
template <bool ERR>
__device__ __forceinline__ double ap_all_bands(const float* __restrict__ P, const float* __restrict__ S, int cs, int nb, int band,
                                               const ApForm& f, double rho, double r0, double c0, int s, const double* s_off,
                                               double* s_red, double* __restrict__ flux, double* __restrict__ err,
                                               double* __restrict__ area) {
  double fa[AP_MAX_BANDS], qa[ERR ? AP_MAX_BANDS : 1], ar[1] = {0.0};
#pragma unroll
  for (int b = 0; b < AP_MAX_BANDS; ++b) fa[b] = 0.0;
#pragma unroll
  for (int b = 0; b < (ERR ? AP_MAX_BANDS : 1); ++b) qa[b] = 0.0;
  ApWalk p(cs, f, rho, r0, c0);
  for (int i = threadIdx.x; i < p.n; i += MS_THREADS, p.next()) {
    const int cnt = ap_count(f, rho, (double)p.row() - r0, (double)p.col() - c0, s, s_off);
    if (cnt > 0) {
      const double w = (double)cnt;
      ar[0] += w;                           // (whole numbers: the sum is exact in any order)
      const long e = (long)p.row() * cs + p.col();
      const float* pp = P + e * nb;
      const float* sp = ERR ? S + e * nb : nullptr;
#pragma unroll
      for (int b = 0; b < AP_MAX_BANDS; ++b) {
        if (b < nb) {
          fa[b] += w * (double)pp[b];
          if (ERR) {
            const double sv = (double)sp[b];
            qa[ERR ? b : 0] += w * (sv * sv);
          }
        }
      }
    }
  }
  ms_block_sum<1>(ar, s_red);
  const double s2 = (double)(s * s);
  if (threadIdx.x == 0) *area = ar[0] / s2;
  double fband = 0.0;
#pragma unroll
  for (int b = 0; b < AP_MAX_BANDS; ++b) {
    if (b < nb) {                           // (nb is uniform: every thread takes the same barriers)
      if (ERR) {
        double a[2] = {fa[b], qa[ERR ? b : 0]};
        ms_block_sum<2>(a, s_red);
        if (threadIdx.x == 0) {
          flux[b] = a[0] / s2;
          err[b] = __dsqrt_rn(a[1] / s2);
        }
        if (b == band) fband = a[0] / s2;
      } else {
        double a[1] = {fa[b]};
        ms_block_sum<1>(a, s_red);
        if (threadIdx.x == 0) flux[b] = a[0] / s2;
        if (b == band) fband = a[0] / s2;
      }
    }
  }
  return fband;
}

// does the box of half-extents (hr, hc) about (r0, c0) leave the stamp?  (false for a NaN extent)
__device__ __forceinline__ bool ap_leaves(double r0, double c0, double hr, double hc, double edge) {
  return r0 - hr < -0.5 || r0 + hr > edge || c0 - hc < -0.5 || c0 + hc > edge;
}

// mean / stddev: stamps [n][cs][cs][nb] float32 (stddev read only with ERR); shape [n][5], status [n]: their catalogue rows;
// o: the output rows of the first stamp
template <bool ERR>
__global__ __launch_bounds__(MS_THREADS) void aperture_kernel(const float* __restrict__ mean, const float* __restrict__ stddev,
                                                              const double* __restrict__ shape, const int* __restrict__ status,
                                                              int cs, int nb, int band, ApertureParams par, ApertureRows o) {
  extern __shared__ double s_mem[];
  const int npix = cs * cs, K = par.K, J = par.J, s = par.subsample;
  double* plane = s_mem;                    // [cs][cs]
  double* s_red = plane + npix;             // [MS_RED]
  double* s_off = s_red + MS_RED;           // [12]: the sub-pixel offsets
  double* s_R = s_off + 12;                 // [AP_MAX_RADII]
  double* s_f = s_R + AP_MAX_RADII;         // [AP_MAX_FRACTIONS]
  const long gi = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double* ap_flux = o.ap_flux + gi * K * nb;
  double* ap_err = ERR ? o.ap_err + gi * K * nb : nullptr;
  double* ap_area = o.ap_area + gi * K;
  double* flux_auto = o.flux_auto + gi * nb;
  double* auto_err = ERR ? o.auto_err + gi * nb : nullptr;
  double* kron = o.kron + gi * 3;
  double* flux_rho = o.flux_rho + gi * J;

  // eligibility: the same answer in every thread (all read the same row)
  const double* sh = shape + gi * 5;
  const double r0 = sh[0], c0 = sh[1], Mrr = sh[2], Mrc = sh[3], Mcc = sh[4];
  const int st_in = status[gi];
  const double det = Mrr * Mcc - Mrc * Mrc;
  if ((st_in != 0 && st_in != 2) || !(ms_finite(r0) && ms_finite(c0) && ms_finite(Mrr) && ms_finite(Mrc) && ms_finite(Mcc)) ||
      !(ms_finite(det) && det > 1e-6)) {
    if (threadIdx.x == 0) {
      for (int i = 0; i < K * nb; ++i) {
        ap_flux[i] = nan;
        if (ERR) ap_err[i] = nan;
      }
      for (int k = 0; k < K; ++k) ap_area[k] = nan;
      for (int b = 0; b < nb; ++b) {
        flux_auto[b] = nan;
        if (ERR) auto_err[b] = nan;
      }
      for (int k = 0; k < 3; ++k) kron[k] = nan;
      for (int j = 0; j < J; ++j) flux_rho[j] = nan;
      o.flags[gi] = 0;
      o.status[gi] = 4;
    }
    return;
  }

  // the band plane, the offsets, the radii and the fractions to LDS
  const float* P = mean + gi * npix * nb;
  const float* S = ERR ? stddev + gi * npix * nb : nullptr;
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) plane[e] = (double)P[(long)e * nb + band];   // (read by other threads: the barrier below)
  if (threadIdx.x < 9) s_off[threadIdx.x] = ((double)threadIdx.x + 0.5) / (double)s - 0.5;
  if (threadIdx.x < AP_MAX_RADII) s_R[threadIdx.x] = par.radii[threadIdx.x];
  if (threadIdx.x < AP_MAX_FRACTIONS) s_f[threadIdx.x] = par.fractions[threadIdx.x];
  __syncthreads();

  const double edge = (double)cs - 0.5;
  int flags = 0;

  // 1. the circles
  const ApForm circle = ap_form(1.0, 0.0, 1.0, 1.0, 1.0);
  for (int k = 0; k < K; ++k) {
    const double R = s_R[k];
    if (ap_leaves(r0, c0, R, R, edge)) flags |= 1 << k;
    ap_all_bands<ERR>(P, S, cs, nb, band, circle, R, r0, c0, s, s_off, s_red, ap_flux + k * nb, ERR ? ap_err + k * nb : nullptr,
                      ap_area + k);
  }

  // 2. the Kron radius
  const double sr = __dsqrt_rn(Mrr), sc = __dsqrt_rn(Mcc);       // (NaN for a negative-definite M: such a pass walks the whole stamp)
  const ApForm ell = ap_form(Mcc / det, (-2.0 * Mrc) / det, Mrr / det, sr, sc);
  if (ap_leaves(r0, c0, par.kron_limit * sr, par.kron_limit * sc, edge)) flags |= 1 << 9;
  double r1;
  {
    const double lim2 = par.kron_limit * par.kron_limit;
    double a[2] = {0.0, 0.0};
    ApWalk p(cs, ell, par.kron_limit, r0, c0);
    for (int i = threadIdx.x; i < p.n; i += MS_THREADS, p.next()) {
      const double q = ap_q(ell, (double)p.row() - r0, (double)p.col() - c0);
      if (q <= lim2) {
        const double v = plane[p.row() * cs + p.col()];
        a[0] += __dsqrt_rn(q) * v;
        a[1] += v;
      }
    }
    ms_block_sum<2>(a, s_red);
    r1 = a[0] / a[1];
    if (!(ms_finite(a[1]) && a[1] > 0.0) || !ms_finite(r1)) {
      if (threadIdx.x == 0) {
        for (int b = 0; b < nb; ++b) {
          flux_auto[b] = nan;
          if (ERR) auto_err[b] = nan;
        }
        for (int k = 0; k < 3; ++k) kron[k] = nan;
        for (int j = 0; j < J; ++j) flux_rho[j] = nan;
        o.flags[gi] = flags;
        o.status[gi] = 7;
      }
      return;
    }
  }
  double rho_auto = par.kron_factor * r1;
  if (rho_auto < par.kron_min) {
    rho_auto = par.kron_min;
    flags |= 1 << 10;
  }
  if (ap_leaves(r0, c0, rho_auto * sr, rho_auto * sc, edge)) flags |= 1 << 8;

  // 3. the automatic aperture
  const double fauto = ap_all_bands<ERR>(P, S, cs, nb, band, ell, rho_auto, r0, c0, s, s_off, s_red, flux_auto, auto_err, kron + 2);

  // 4. the flux radii
  for (int j = 0; j < J; ++j) {
    const double t = s_f[j] * fauto;
    double lo = 0.0, hi = rho_auto;
    for (int i = 0; i < par.bisect_iters; ++i) {
      const double mid = 0.5 * (lo + hi);
      if (ap_plane_flux(plane, cs, ell, mid, r0, c0, s, s_off, s_red) >= t) hi = mid;
      else lo = mid;
    }
    if (threadIdx.x == 0) flux_rho[j] = hi;
  }
  if (threadIdx.x == 0) {
    kron[0] = r1;
    kron[1] = rho_auto;
    o.flags[gi] = flags;
    o.status[gi] = 0;
  }
}

// ---- the same apertures on the fields ------------------------------------------------------------------------
// One aperture in every band of the completed mean field T and the observed field D of the galaxy's field (both [F][F][nb]
// float64, the galaxy's stamp placed at (pr, pc)): msum [nb], dsum [nb] (NaN without DATA), *area by thread 0.  The walk is
// ap_all_bands': the same box, the same assignment of pixels to threads, the same count; a pixel whose field pixel lies outside
// the field is skipped (the composite dropped it).  A pixel of positive count reads the nb contiguous doubles of T and of D.
// Where T holds a stamp's widened values and no pixel is skipped, the additions are those of ap_all_bands in its order.
template <bool DATA>
__device__ __forceinline__ void ap_field_bands(const double* __restrict__ T, const double* __restrict__ D, int cs, int nb, int F,
                                               int pr, int pc, const ApForm& f, double rho, double r0, double c0, int s,
                                               const double* s_off, double* s_red, double* __restrict__ msum,
                                               double* __restrict__ dsum, double* __restrict__ area) {
  double ta[AP_MAX_BANDS], da[DATA ? AP_MAX_BANDS : 1], ar[1] = {0.0};
#pragma unroll
  for (int b = 0; b < AP_MAX_BANDS; ++b) ta[b] = 0.0;
#pragma unroll
  for (int b = 0; b < (DATA ? AP_MAX_BANDS : 1); ++b) da[b] = 0.0;
  ApWalk p(cs, f, rho, r0, c0);
  for (int i = threadIdx.x; i < p.n; i += MS_THREADS, p.next()) {
    const int fr = pr + p.row(), fc = pc + p.col();
    if ((unsigned)fr >= (unsigned)F || (unsigned)fc >= (unsigned)F) continue;
    const int cnt = ap_count(f, rho, (double)p.row() - r0, (double)p.col() - c0, s, s_off);
    if (cnt > 0) {
      const double w = (double)cnt;
      ar[0] += w;                           // (whole numbers: the sum is exact in any order)
      const long e = ((long)fr * F + fc) * nb;
      const double* tp = T + e;
      const double* dp = DATA ? D + e : nullptr;
#pragma unroll
      for (int b = 0; b < AP_MAX_BANDS; ++b) {
        if (b < nb) {
          ta[b] += w * tp[b];
          if (DATA) da[DATA ? b : 0] += w * dp[b];
        }
      }
    }
  }
  ms_block_sum<1>(ar, s_red);
  const double s2 = (double)(s * s);
  if (threadIdx.x == 0) *area = ar[0] / s2;
#pragma unroll
  for (int b = 0; b < AP_MAX_BANDS; ++b) {
    if (b < nb) {                           // (nb is uniform: every thread takes the same barriers)
      if (DATA) {
        double a[2] = {ta[b], da[DATA ? b : 0]};
        ms_block_sum<2>(a, s_red);
        if (threadIdx.x == 0) {
          msum[b] = a[0] / s2;
          dsum[b] = a[1] / s2;
        }
      } else {
        double a[1] = {ta[b]};
        ms_block_sum<1>(a, s_red);
        if (threadIdx.x == 0) {
          msum[b] = a[0] / s2;
          dsum[b] = __longlong_as_double(0x7ff8000000000000LL);
        }
      }
    }
  }
}

// shape [n][5], status [n], kron [n][3], aper_status [n], places [n][2], sfield [n]: the rows of n galaxies whose fields are
// complete; model / data: the stacks from field f0 on (data read only with DATA); o: the output rows of the first galaxy.
// LDS: the reduction scratch, the sub-pixel offsets and the radii - no plane
template <bool DATA>
__global__ __launch_bounds__(MS_THREADS) void aperture_field_kernel(const double* __restrict__ shape, const int* __restrict__ status,
                                                                    const double* __restrict__ kron,
                                                                    const int* __restrict__ aper_status,
                                                                    const int* __restrict__ places, const int* __restrict__ sfield,
                                                                    int f0, int cs, int nb, int F, const double* __restrict__ model,
                                                                    const double* __restrict__ data, ApertureParams par,
                                                                    ApertureFieldRows o) {
  __shared__ double s_red[MS_RED];
  __shared__ double s_off[12];
  __shared__ double s_R[AP_MAX_RADII];
  const int K = par.K, s = par.subsample;
  const long gi = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double* ap_model = o.ap_model + gi * K * nb;
  double* ap_data = o.ap_data + gi * K * nb;
  double* ap_farea = o.ap_farea + gi * K;
  double* auto_model = o.auto_model + gi * nb;
  double* auto_data = o.auto_data + gi * nb;

  // eligibility: the same answer in every thread (all read the same rows)
  const double* sh = shape + gi * 5;
  const double r0 = sh[0], c0 = sh[1], Mrr = sh[2], Mrc = sh[3], Mcc = sh[4];
  const int st_in = status[gi], ast = aper_status[gi];
  const double det = Mrr * Mcc - Mrc * Mrc;
  const bool row_ok = ast != 4 && (st_in == 0 || st_in == 2) &&
                      (ms_finite(r0) && ms_finite(c0) && ms_finite(Mrr) && ms_finite(Mrc) && ms_finite(Mcc)) &&
                      (ms_finite(det) && det > 1e-6);
  if (!row_ok || ast != 0) {
    if (threadIdx.x == 0) {
      if (!row_ok) {
        for (int i = 0; i < K * nb; ++i) ap_model[i] = ap_data[i] = nan;
        for (int k = 0; k < K; ++k) ap_farea[k] = nan;
      }
      for (int b = 0; b < nb; ++b) auto_model[b] = auto_data[b] = nan;
      o.auto_farea[gi] = nan;
    }
    if (!row_ok) return;
  }

  if (threadIdx.x < 9) s_off[threadIdx.x] = ((double)threadIdx.x + 0.5) / (double)s - 0.5;
  if (threadIdx.x < AP_MAX_RADII) s_R[threadIdx.x] = par.radii[threadIdx.x];
  __syncthreads();

  const int pr = places[2 * gi], pc = places[2 * gi + 1];
  const long fo = (long)(sfield[gi] - f0) * F * F * nb;
  const double* T = model + fo;
  const double* D = DATA ? data + fo : nullptr;

  const ApForm circle = ap_form(1.0, 0.0, 1.0, 1.0, 1.0);
  for (int k = 0; k < K; ++k)
    ap_field_bands<DATA>(T, D, cs, nb, F, pr, pc, circle, s_R[k], r0, c0, s, s_off, s_red, ap_model + k * nb, ap_data + k * nb,
                         ap_farea + k);
  if (ast != 0) return;                     // (no Kron radius: the circles alone)
  const ApForm ell = ap_form(Mcc / det, (-2.0 * Mrc) / det, Mrr / det, __dsqrt_rn(Mrr), __dsqrt_rn(Mcc));
  ap_field_bands<DATA>(T, D, cs, nb, F, pr, pc, ell, kron[gi * 3 + 1], r0, c0, s, s_off, s_red, auto_model, auto_data,
                       o.auto_farea + gi);
}
}  // namespace

size_t aperture_lds_bytes(int cs) { return ((size_t)cs * cs + AP_SCRATCH) * sizeof(double); }

// the refusals of the aperture photometry, before any GPU work
int aperture_check(const char* who, int cs, int nb, int band, const ApertureParams& p) {
  if (cs < 1 || nb < 1 || nb > AP_MAX_BANDS) {
    set_error("%s: stamps of %d pixels and %d bands; the aperture photometry takes 1 .. %d bands", who, cs, nb, AP_MAX_BANDS);
    return E_INVALID;
  }
  if (cs > 4096 || aperture_lds_bytes(cs) > AP_LDS_BUDGET) {
    set_error("%s: the %d x %d band plane (%zu bytes as float64) does not fit the %zu bytes of LDS the aperture kernel uses: "
              "stamps of at most 90 pixels", who, cs, cs, (size_t)cs * cs * sizeof(double), AP_LDS_BUDGET);
    return E_INVALID;
  }
  if (band < 0 || band >= nb) {
    set_error("%s: band %d asked for, the stamps have bands 0 .. %d", who, band, nb - 1);
    return E_INVALID;
  }
  if (p.K < 0 || p.K > AP_MAX_RADII || p.J < 0 || p.J > AP_MAX_FRACTIONS) {
    set_error("%s: %d aperture radii and %d flux fractions; 0 .. %d radii and 0 .. %d fractions are taken", who, p.K, p.J,
              AP_MAX_RADII, AP_MAX_FRACTIONS);
    return E_INVALID;
  }
  for (int k = 0; k < p.K; ++k) {
    if (!(std::isfinite(p.radii[k]) && p.radii[k] > 0.0)) {
      set_error("%s: aperture radius %d must be finite and positive (got %g)", who, k, p.radii[k]);
      return E_INVALID;
    }
  }
  for (int j = 0; j < p.J; ++j) {
    if (!(p.fractions[j] > 0.0 && p.fractions[j] < 1.0)) {
      set_error("%s: flux fraction %d must lie strictly between 0 and 1 (got %g)", who, j, p.fractions[j]);
      return E_INVALID;
    }
  }
  if (p.subsample < 1 || p.subsample > 9 || p.bisect_iters < 1 || p.bisect_iters > 60) {
    set_error("%s: subsample must be 1 .. 9 and bisect_iters 1 .. 60 (got %d, %d)", who, p.subsample, p.bisect_iters);
    return E_INVALID;
  }
  if (!(std::isfinite(p.kron_factor) && p.kron_factor > 0.0) || !(std::isfinite(p.kron_min) && p.kron_min > 0.0) ||
      !(std::isfinite(p.kron_limit) && p.kron_limit > 0.0)) {
    set_error("%s: kron_factor, kron_min and kron_limit must be finite and positive (got %g, %g, %g)", who, p.kron_factor,
              p.kron_min, p.kron_limit);
    return E_INVALID;
  }
  return OK;
}

// the outputs a call with these parameters must give (err: with a stddev stamp); n == 0 needs none
int aperture_rows_check(const char* who, const ApertureRows& o, const ApertureParams& p, bool err, int64_t n) {
  if (n <= 0) return OK;
  const bool circles = p.K == 0 || (o.ap_flux && o.ap_area && (!err || o.ap_err));
  if (!circles || !o.flux_auto || (err && !o.auto_err) || !o.kron || (p.J > 0 && !o.flux_rho) || !o.flags || !o.status) {
    set_error("%s: ap_flux, ap_area (with radii), flux_auto, kron, flux_rho (with fractions), aper_flags and aper_status must "
              "all be given%s", who, err ? ", and ap_flux_err and flux_auto_err with them" : "");
    return E_INVALID;
  }
  return OK;
}

// the columns of the aperture rows: the circles only with radii, the errors only with a stddev stamp, flux_rho only with
// fractions
void aperture_columns(Rows& r, ApertureRows& dev, const ApertureRows& host, const ApertureParams& p, int nb, bool err) {
  if (p.K > 0) {
    r.add(dev.ap_flux, host.ap_flux, (size_t)p.K * nb);
    r.add(dev.ap_area, host.ap_area, p.K);
    if (err) r.add(dev.ap_err, host.ap_err, (size_t)p.K * nb);
  }
  r.add(dev.flux_auto, host.flux_auto, nb);
  if (err) r.add(dev.auto_err, host.auto_err, nb);
  r.add(dev.kron, host.kron, 3);
  if (p.J > 0) r.add(dev.flux_rho, host.flux_rho, p.J);
  r.add(dev.flags, host.flags, 1);
  r.add(dev.status, host.status, 1);
}

// the rows of `o` that start at stamp r
ApertureRows aperture_rows_at(const ApertureRows& o, int64_t r, const ApertureParams& p, int nb) {
  ApertureRows v = o;
  Rows c;
  aperture_columns(c, v, ApertureRows{}, p, nb, o.auto_err != nullptr);
  c.advance(r);
  return v;
}

// n stamps that lie in device memory with their catalogue rows; every per-galaxy pointer is the row of the first stamp
// (stddev_dev is read only where the rows have ap_err and auto_err)
int launch_aperture(const float* mean_dev, const float* stddev_dev, const double* shape_dev, const int* status_dev, int n, int cs,
                    int nb, int band, const ApertureParams& p, const ApertureRows& rows, hipStream_t s) {
  if (n <= 0) return OK;
  const size_t smem = aperture_lds_bytes(cs);
  if (stddev_dev && rows.auto_err)
    hipLaunchKernelGGL(aperture_kernel<true>, dim3((unsigned)n), dim3(MS_THREADS), smem, s, mean_dev, stddev_dev, shape_dev,
                       status_dev, cs, nb, band, p, rows);
  else
    hipLaunchKernelGGL(aperture_kernel<false>, dim3((unsigned)n), dim3(MS_THREADS), smem, s, mean_dev, stddev_dev, shape_dev,
                       status_dev, cs, nb, band, p, rows);
  DV_HIP(hipGetLastError());
  return OK;
}

// host arrays in, host rows out, a chunk of stamps at a time
int scene_aperture(const float* mean_h, const float* stddev_h, const double* shape_h, const int32_t* status_h, int64_t N, int cs,
                   int nb, int band, const ApertureParams& p, const ApertureRows& out_h, hipStream_t s) {
  const char* who = "dv_scene_aperture";
  DV_TRY(aperture_check(who, cs, nb, band, p));
  if (N < 0 || (N > 0 && (!mean_h || !shape_h || !status_h))) {
    set_error("%s: mean, shape and status must all be given", who);
    return E_INVALID;
  }
  DV_TRY(aperture_rows_check(who, out_h, p, stddev_h != nullptr, N));
  if ((stddev_h == nullptr) != (out_h.auto_err == nullptr) || (p.K > 0 && (stddev_h == nullptr) != (out_h.ap_err == nullptr))) {
    set_error("%s: stddev, ap_flux_err and flux_auto_err go together (all given or all null)", who);
    return E_INVALID;
  }
  const size_t stamp = (size_t)cs * cs * nb;
  float *mean = nullptr, *sd = nullptr;
  double* shape = nullptr;
  int* status = nullptr;
  ApertureRows d{};
  Rows in, out;
  in.add(mean, mean_h, stamp);
  if (stddev_h) in.add(sd, stddev_h, stamp);
  in.add(shape, shape_h, 5);
  in.add(status, status_h, 1);
  aperture_columns(out, d, out_h, p, nb, stddev_h != nullptr);
  return walk_rows(N, (int64_t)1 << 20, 0, in, out, s,
                   [&](int64_t, int n) { return launch_aperture(mean, sd, shape, status, n, cs, nb, band, p, d, s); });
}

// ---- the same apertures on the fields: host side ---------------------------------------------------------------
// the outputs a call with these parameters must give; n == 0 needs none
int aperture_field_rows_check(const char* who, const ApertureFieldRows& o, const ApertureParams& p, int64_t n) {
  if (n <= 0) return OK;
  const bool circles = p.K == 0 || (o.ap_model && o.ap_data && o.ap_farea);
  if (!circles || !o.auto_model || !o.auto_data || !o.auto_farea) {
    set_error("%s: ap_model_sum, ap_data_sum, ap_field_area (with radii), auto_model_sum, auto_data_sum and auto_field_area must "
              "all be given", who);
    return E_INVALID;
  }
  return OK;
}

void aperture_field_columns(Rows& r, ApertureFieldRows& dev, const ApertureFieldRows& host, const ApertureParams& p, int nb) {
  if (p.K > 0) {
    r.add(dev.ap_model, host.ap_model, (size_t)p.K * nb);
    r.add(dev.ap_data, host.ap_data, (size_t)p.K * nb);
    r.add(dev.ap_farea, host.ap_farea, p.K);
  }
  r.add(dev.auto_model, host.auto_model, nb);
  r.add(dev.auto_data, host.auto_data, nb);
  r.add(dev.auto_farea, host.auto_farea, 1);
}

// the rows of `o` that start at galaxy r
ApertureFieldRows aperture_field_rows_at(const ApertureFieldRows& o, int64_t r, const ApertureParams& p, int nb) {
  ApertureFieldRows v = o;
  Rows c;
  aperture_field_columns(c, v, ApertureFieldRows{}, p, nb);
  c.advance(r);
  return v;
}

// n galaxies whose fields are complete, with their catalogue and aperture rows, placements and fields in device memory; every
// per-galaxy pointer is the row of the first galaxy
int launch_aperture_field(const double* shape_dev, const int* status_dev, const double* kron_dev, const int* aper_status_dev,
                          const int* places_dev, const int* sfield_dev, int f0, int n, int cs, int nb, int F,
                          const double* model_dev, const double* data_dev, const ApertureParams& p,
                          const ApertureFieldRows& rows, hipStream_t s) {
  if (n <= 0) return OK;
  if (data_dev)
    hipLaunchKernelGGL(aperture_field_kernel<true>, dim3((unsigned)n), dim3(MS_THREADS), 0, s, shape_dev, status_dev, kron_dev,
                       aper_status_dev, places_dev, sfield_dev, f0, cs, nb, F, model_dev, data_dev, p, rows);
  else
    hipLaunchKernelGGL(aperture_field_kernel<false>, dim3((unsigned)n), dim3(MS_THREADS), 0, s, shape_dev, status_dev, kron_dev,
                       aper_status_dev, places_dev, sfield_dev, f0, cs, nb, F, model_dev, data_dev, p, rows);
  DV_HIP(hipGetLastError());
  return OK;
}

// host arrays in, host rows out: a chunk of galaxies at a time, the model (and data) fields they lie in uploaded beside
// their rows
int scene_aperture_fields(const double* shape_h, const int32_t* status_h, const int32_t* places_h, const int64_t* field_ptr,
                          const double* kron_h, const int32_t* aper_status_h, int64_t N, int cs, int nb, const double* model_h,
                          const double* data_h, int M, int F, const ApertureParams& p, const ApertureFieldRows& out_h,
                          int device, hipStream_t s) {
  const char* who = "dv_scene_aperture_fields";
  DV_TRY(aperture_check(who, cs, nb, 0, p));
  if (N < 0 || M < 0 || !field_ptr ||
      (N > 0 && (!shape_h || !status_h || !places_h || !kron_h || !aper_status_h || !model_h))) {
    set_error("%s: shape, status, places, field_ptr, kron, aper_status and model_fields must all be given", who);
    return E_INVALID;
  }
  DV_TRY(aperture_field_rows_check(who, out_h, p, N));
  std::vector<int32_t> sfield;                       // every galaxy's field
  DV_TRY(field_tables(who, "galaxies", M, field_ptr, N, &F, places_h, &sfield, nullptr));
  if (N == 0) return OK;
  DV_HIP(hipSetDevice(device));
  double *shape = nullptr, *kron = nullptr;
  int *status = nullptr, *astatus = nullptr, *places = nullptr, *sf = nullptr;
  ApertureFieldRows d{};
  Rows in, out;
  in.add(shape, shape_h, 5);
  in.add(kron, kron_h, 3);
  in.add(status, status_h, 1);
  in.add(astatus, aper_status_h, 1);
  in.add(places, places_h, 2);
  in.add(sf, sfield.data(), 1);
  aperture_field_columns(out, d, out_h, p, nb);
  FieldStacks f{model_h, data_h, (size_t)F * F * nb, M};
  return walk_field_rows(N, sfield.data(), f, in, out, s, [&](int64_t, int n, int fa) {
    return launch_aperture_field(shape, status, kron, astatus, places, sf, fa, n, cs, nb, F, f.model_d, f.data_d, p, d, s);
  });
}

}  // namespace dv
