// Device pieces the measurement kernels share (measure.hip, blend.hip, regauss.hip, aperture.hip, fitflux.hip): the workgroup
// reduction and the adaptive-moments iteration of DESIGN.md 7j on a float64 plane that lies in LDS.  Everything is inlined into the kernel that calls it.
#pragma once
#include "common.h"

namespace dv {

constexpr int MS_THREADS = 256;
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

// The iteration on plane [cs][cs] from the state (r0, c0, Mrr, Mrc, Mcc), which it updates; returns the iterations taken in
// `it` and the status in `st`.  Every thread reads only the plane elements e = threadIdx.x + k MS_THREADS (a caller whose
// threads wrote those same elements needs no barrier before it) and every thread ends with the same state.
__device__ __forceinline__ void ms_iterate(const double* plane, int cs, double tol, int max_iter, double& r0, double& c0,
                                           double& Mrr, double& Mrc, double& Mcc, int& it, int& st, double* s_red) {
  const int npix = cs * cs;
  const double ctr = 0.5 * (double)(cs - 1), half = 0.5 * (double)cs;
  it = 0;
  st = 2;
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
}

}  // namespace dv
