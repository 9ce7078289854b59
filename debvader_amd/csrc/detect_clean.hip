// The cleaning pass of the detector (tests/detect_clean_oracle.py): after SExtractor's clean.c, an object
// that would not have been detected without the extrapolated wings of a brighter neighbour is merged into that neighbour.
// It runs behind the deblend launch and seg_base_kernel on one launch's raw objects, the rows of the catalogue in order:
//  1. clean_mthresh_kernel  one workgroup per raw object: the minarea-th largest D - T over the object's pixels (a scan of its
//                           box in D / segmap per round, every round one block maximum below the last with its count of
//                           ties), then the object's ellipse and the Moffat profile's amp and alpha.
//  2. clean_pairs_kernel    one workgroup per object i, threads stride the objects j of i's field: the profile of j at i
//                           against mthresh_i, the largest one (ties to the smaller row) is absorber[i].
//  3. clean_root_kernel     one workgroup per field: pointer jumping from one array into the other until a sweep changes
//                           nothing, then the survivors' new row numbers in order (block scans).
//  4. clean_segmap_kernel   one thread per pixel: old number -> new number.
// Every test reads the raw values, so the result does not depend on the order of threads or launches.  Ordinary vector
// stores, no atomics.  The merge of the rows themselves is O(n) and stays on the host (detect.hip, append_catalogue).
#include "common.h"

#pragma clang fp contract(off)

#include "deblend_dev.h"

namespace dv {

namespace {
constexpr double CLEAN_PI = 3.141592653589793;
constexpr double CLEAN_ZONE2 = 100.0;      // SExtractor's CLEAN_ZONE of 10, squared

// max of v over the workgroup; every thread gets the result (s_v: one double per wave)
__device__ __forceinline__ double blk_dmax(double v, double* s_v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) s_v[wave] = v;
  __syncthreads();
  return fmax(fmax(s_v[0], s_v[1]), fmax(s_v[2], s_v[3]));
}

__global__ __launch_bounds__(DT) void clean_mthresh_kernel(CleanTables t, int minarea, double beta) {
  __shared__ double s_v[4];
  __shared__ int s_w[4];
  const int tid = threadIdx.x;
  const int i = (int)blockIdx.x;
  const int f = t.rfield[i], num = t.rnum[i];
  const double T = t.fT[f];
  const int c0 = t.rbox[4 * (long)i], c1 = t.rbox[4 * (long)i + 1], r0 = t.rbox[4 * (long)i + 2], r1 = t.rbox[4 * (long)i + 3];
  const double* Df = t.D + (long)f * t.HW;
  const int* segf = t.seg + (long)f * t.HW;
  const int bw = c1 - c0 + 1;
  const long total = (long)(r1 - r0 + 1) * bw;
  double bound = INFINITY, res = 0.0;
  int cum = 0;
  if (t.rnpix[i] >= minarea) {
    for (int round = 0; round < minarea; ++round) {          // (every quantity of the loop's control is uniform)
      double m = -INFINITY;
      int c = 0;
      for (long e = tid; e < total; e += DT) {
        const long p = (long)(r0 + (int)(e / bw)) * t.W + c0 + (int)(e % bw);
        if (segf[p] != num) continue;
        const double d = Df[p] - T;
        if (!(d < bound)) continue;
        if (d > m) { m = d; c = 1; }
        else if (d == m) ++c;
      }
      const double bm = blk_dmax(m, s_v);
      if (!(bm > -INFINITY)) break;                           // no value is left below the bound
      cum += blk_isum(m == bm ? c : 0, s_w);
      if (cum >= minarea) { res = bm; break; }
      bound = bm;
    }
  }
  if (tid == 0) {
    const double* rd = t.rd + 6 * (long)i;
    const double dflux = rd[0], x2 = rd[3], y2 = rd[4], xy = rd[5];
    const double det = x2 * y2 - xy * xy;
    const double area = CLEAN_PI * sqrt(det);
    const double hd = (x2 - y2) / 2.0;
    const double amp = dflux / (2.0 * area);
    double* o = t.der + 6 * (long)i;
    o[0] = sqrt((x2 + y2) / 2.0 + sqrt(hd * hd + xy * xy));  // a
    o[1] = amp;
    o[2] = (pow(amp / T, 1.0 / beta) - 1.0) * area / (double)t.rnpix[i];   // alpha
    o[3] = y2 / det;                                         // cxx
    o[4] = x2 / det;                                         // cyy
    o[5] = -2.0 * xy / det;                                  // cxy
    t.mthresh[i] = res;
  }
}

__global__ __launch_bounds__(DT) void clean_pairs_kernel(CleanTables t, double beta) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  const int tid = threadIdx.x;
  const int i = (int)blockIdx.x;
  const int f = t.rfield[i];
  const int lo = t.fptr[f], hi = t.fptr[f + 1];
  const double T = t.fT[f];
  const double dfi = t.rd[6 * (long)i], xi = t.rd[6 * (long)i + 1], yi = t.rd[6 * (long)i + 2];
  const double ai = t.der[6 * (long)i], mth = t.mthresh[i];
  double best = -INFINITY;
  int bj = 0x7fffffff;
  if (T > 0.0) {
    for (int j = lo + tid; j < hi; j += DT) {
      if (j == i) continue;
      const double dfj = t.rd[6 * (long)j];
      if (!(dfj > dfi || (dfj == dfi && j < i))) continue;
      const double* dj = t.der + 6 * (long)j;
      const double dx = xi - t.rd[6 * (long)j + 1], dy = yi - t.rd[6 * (long)j + 2];
      const double sa = ai + dj[0];
      if (!(dx * dx + dy * dy < CLEAN_ZONE2 * (sa * sa))) continue;
      const double val = 1.0 + dj[2] * ((dj[3] * dx) * dx + (dj[4] * dy) * dy + (dj[5] * dx) * dy);
      const double P = (val > 1.0 && val < 1e10) ? dj[1] * pow(val, -beta) : 0.0;
      if (!(P > mth)) continue;
      if (P > best || (P == best && j < bj)) { best = P; bj = j; }
    }
  }
  blk_argmax(best, bj, s_v, s_i);
  if (tid == 0) t.absorber[i] = bj == 0x7fffffff ? i : bj;
}

// root [2][n]: the two arrays of the sweeps; newrow[i]: the row of i's root among the survivors of its field
__global__ __launch_bounds__(DT) void clean_root_kernel(CleanTables t) {
  __shared__ int s_changed;
  __shared__ int s_w[4];
  const int tid = threadIdx.x;
  const int f = (int)blockIdx.x;
  const int lo = t.fptr[f], n = t.fptr[f + 1] - lo;
  int* A = t.root + lo;
  int* B = t.root + (long)t.n + lo;
  for (int i = tid; i < n; i += DT) A[i] = t.absorber[lo + i] - lo;
  if (tid == 0) s_changed = 0;
  __syncthreads();
  for (;;) {
    int changed = 0;
    for (int i = tid; i < n; i += DT) {
      const int old = A[i];
      const int l = A[old];
      B[i] = l;
      changed |= l != old;
    }
    if (changed) s_changed = 1;              // (every writer writes the same value)
    __syncthreads();
    const bool again = s_changed != 0;       // (uniform)
    __syncthreads();                         // everyone has read the flag
    if (tid == 0) s_changed = 0;
    __syncthreads();                         // the flag is clear before the next sweep sets it
    int* x = A;
    A = B;
    B = x;
    if (!again) break;
  }
  // the survivors in order: B takes their new rows, then every object reads its root's
  int count = 0;
  for (int base = 0; base < n; base += DT) {
    const int i = base + tid;
    const bool sv = i < n && A[i] == i;
    int tot;
    const int at = count + blk_scan(sv ? 1 : 0, s_w, tot);
    if (sv) B[i] = at;
    count += tot;
  }
  __syncthreads();
  for (int i = tid; i < n; i += DT) {
    t.rootout[lo + i] = lo + A[i];
    t.newrow[lo + i] = B[A[i]];
  }
  if (tid == 0) t.nsurv[f] = count;
}

__global__ __launch_bounds__(DT) void clean_segmap_kernel(CleanTables t, int* __restrict__ seg, long total) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const int v = seg[e];
  if (v > 0) seg[e] = t.newrow[t.fptr[e / t.HW] + v - 1] + 1;
}
}  // namespace

int detect_clean_launch(const CleanTables& t, int* seg, long px, int minarea, double beta, hipStream_t s) {
  if (t.n <= 0) return OK;
  hipLaunchKernelGGL(clean_mthresh_kernel, dim3((unsigned)t.n), dim3(DT), 0, s, t, minarea, beta);
  DV_HIP(hipGetLastError());
  hipLaunchKernelGGL(clean_pairs_kernel, dim3((unsigned)t.n), dim3(DT), 0, s, t, beta);
  DV_HIP(hipGetLastError());
  hipLaunchKernelGGL(clean_root_kernel, dim3((unsigned)t.nf), dim3(DT), 0, s, t);
  DV_HIP(hipGetLastError());
  hipLaunchKernelGGL(clean_segmap_kernel, dim3((unsigned)((px + DT - 1) / DT)), dim3(DT), 0, s, t, seg, px);
  DV_HIP(hipGetLastError());
  return OK;
}

}  // namespace dv
