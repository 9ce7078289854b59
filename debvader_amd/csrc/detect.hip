// Source detection (reference: detect/detection.py, which calls sep), batched over fields, float64 throughout.
//
// SExtractor's published method (Bertin & Arnouts 1996) with the rules of DESIGN.md section 7e; tests/detect_oracle.py is
// the same definition in numpy.  Per chunk of fields:
//  1. bkg_mesh_kernel    one workgroup per mesh (<= 64 x 64 values): bitonic sort in LDS, then every kept set of the
//                        sigma clipping is a contiguous range of the sorted values (two binary searches and two fixed-order
//                        reductions per round).
//  2. bkg_grid_kernel    one workgroup per field: median filter over the meshes, globalrms, spline second derivatives along
//                        the mesh rows.
//  3. bkg_row_kernel     one thread per pixel row: the mesh-row splines at that row, then the spline along the columns.
//  4. bkg_pixel_kernel   back (and rms) per pixel, v = data - back.
//  5. filter_kernel      16 x 16 output tiles with the kernel's halo in LDS: D, and the segmentation's initial parents.
//  6. cc_merge_kernel    8-connected union-find over the field on a global parent array: links always go from the larger
//                        root to the smaller (atomic min), so every root is the smallest raster index of its component
//                        whatever the dispatch order.  Parents other threads write in the same launch are read with relaxed
//                        agent-scope atomics.  cc_flatten_kernel (next launch) writes the labels, areas and bounding boxes.
//  7. cc_compact_kernel  one workgroup per field: the components of >= minarea pixels in root order (block scans).
//  8. deblend_kernel     one workgroup per component: pixel list in raster order (scan of the bounding box), the nthresh - 1
//                        levels with a union-find per level, the decision rule, the argmax assignment and the catalog, each
//                        reduction in a fixed order.  Components of <= DB_LDS pixels keep their hot arrays in LDS, larger ones
//                        run the same code on global scratch.
// The catalog is sized in two phases: the component table comes back to the host, which places every component's
// scratch and catalog slots (an object holds >= minarea core pixels, so a component has at most n / minarea of them).
// With a per-pixel noise map and a mask (tests/detect_weighted_oracle.py) kernels 1, 2, 4 and 5 run
// in their WEIGHTED instantiations: only counting pixels (0 < w < inf) enter the meshes, bad meshes are filled from their
// nearest good ones, v is 0 under the mask and D holds the significance S; kernels 6 to 8 read S where they read D.
// On the inverse-variance combination of several bands (tests/detect_multiband_oracle.py)
// bands_gather_kernel writes the selected planes of the interleaved fields, kernels 1 to 3 run over fields x bands planes,
// multiband_pixel_kernel stands where kernel 4 stood and writes the combined v and its weight, and kernel 5 runs WEIGHTED on them.
// With the object columns or the segmentation map asked for (tests/detect_objects_oracle.py) kernel 8 runs
// in its OBJECTS instantiation (deblend_dev.h, launched from detect_objects.hip): step e also takes every object's box, peak
// pixels, isophotal moments and flags and numbers the object's pixels within the component; seg_base_kernel adds the objects of
// the field's earlier components.
// With the cleaning pass (tests/detect_clean_oracle.py) the four kernels of detect_clean.hip run behind
// seg_base_kernel on the launch's raw objects; the merge of the rows is the host's (append_catalogue).
// fp64 VALU and integer work; nothing here has a matrix shape for MFMA.
#include "common.h"
#include "../../include/debvader_hip.h"   // dv_detect_params

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

// Every multiply and add is rounded on its own, as in the numpy restatement (tests/detect_oracle.py): a contracted FMA
// could move a D value across the threshold or reorder two near-equal assignment scores.
#pragma clang fp contract(off)

#include "deblend_dev.h"

namespace dv {

namespace {
constexpr int MESH_MAX = 4096;       // back_size <= 64
constexpr int MF_MAX = 7;            // back_filter <= 7
constexpr int KMAX = 15;             // filter kernels up to 15 x 15
constexpr int FT = 16;               // filter output tile
constexpr int DIM_MAX = 1 << 19;     // H, W (filter grid rows)
constexpr int CHUNK_MAX = 65535;     // fields per launch (filter grid z)

// ---- background --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double median_sorted(const double* s, int n) {
  return (n & 1) ? s[n / 2] : 0.5 * (s[n / 2 - 1] + s[n / 2]);
}


// WEIGHTED (7z): only the counting pixels of wt enter the clipping, a mesh with fewer than half of its pixels counting is
// marked bad with NaN
template <bool WEIGHTED>
__global__ __launch_bounds__(DT) void bkg_mesh_kernel(const double* __restrict__ data, const double* __restrict__ wt, int H,
                                                      int W, int bs, int ny, int nx, double* __restrict__ mback,
                                                      double* __restrict__ mrms) {
  __shared__ double s[MESH_MAX];
  __shared__ double s_red[4];
  __shared__ int s_w[4];
  const int tid = threadIdx.x;
  const long mesh = blockIdx.x;
  const int per = ny * nx;
  const long f = mesh / per;
  const int mi = (int)(mesh - f * per), i = mi / nx, j = mi - (mi / nx) * nx;
  const int r0 = i * bs, c0 = j * bs;
  const int bh = min(bs, H - r0), bw = min(bs, W - c0);
  const int nall = bh * bw;
  int N = 1;
  while (N < nall) N <<= 1;
  const double* src = data + f * (long)H * W;
  int n = nall;
  if constexpr (WEIGHTED) {
    // a pixel that does not count sorts behind every value: the first n sorted values are the counting ones
    const double* wsrc = wt + f * (long)H * W;
    int mine = 0;
    for (int e = tid; e < N; e += DT) {
      bool on = false;
      long at = 0;
      if (e < nall) {
        at = (long)(r0 + e / bw) * W + c0 + e % bw;
        on = counts(wsrc[at]);
      }
      s[e] = on ? src[at] : INFINITY;
      mine += on;
    }
    n = blk_isum(mine, s_w);
    if (2 * n < nall) {                            // a bad mesh (the same for every thread): bkg_grid_kernel fills it
      if (tid == 0) {
        mback[mesh] = NAN;
        mrms[mesh] = NAN;
      }
      return;
    }
  } else {
    for (int e = tid; e < N; e += DT) s[e] = e < nall ? src[(long)(r0 + e / bw) * W + c0 + e % bw] : INFINITY;
  }
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1) {            // bitonic sort, ascending
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int e = tid; e < N; e += DT) {
        const int p = e ^ jj;
        if (p > e) {
          const double a = s[e], b = s[p];
          if ((e & k) == 0 ? a > b : a < b) { s[e] = b; s[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  int lo = 0, hi = n;
  double mean = 0.0, sig = 0.0, med = 0.0;
  for (int round = 0; round <= 100; ++round) {
    const int m = hi - lo;
    double a[1] = {0.0};
    for (int e = lo + tid; e < hi; e += DT) a[0] += s[e];
    blk_sum<1>(a, s_red);
    mean = a[0] / m;
    double b[1] = {0.0};
    for (int e = lo + tid; e < hi; e += DT) {
      const double d = s[e] - mean;
      b[0] += d * d;
    }
    blk_sum<1>(b, s_red);
    sig = sqrt(b[0] / m);
    med = median_sorted(s + lo, m);
    if (round == 100) break;                       // the statistics of the set after 100 rounds
    const double la = med - 3.0 * sig, ha = med + 3.0 * sig;
    int l = lo, h = hi;
    while (l < h) { const int c = (l + h) >> 1; if (s[c] < la) l = c + 1; else h = c; }
    const int nlo = l;
    l = lo; h = hi;
    while (l < h) { const int c = (l + h) >> 1; if (s[c] <= ha) l = c + 1; else h = c; }
    const int nhi = l;
    if (nlo == lo && nhi == hi) break;            // the kept set did not change: these are its statistics
    lo = nlo;
    hi = nhi;
  }
  if (tid == 0) {
    mback[mesh] = fabs(mean - med) < 0.3 * sig ? 2.5 * med - 1.5 * mean : med;
    mrms[mesh] = sig;
  }
}

// second derivatives of the natural cubic spline through y[0], y[st], ... (n values, unit spacing) into m (same stride);
// cco[i] = the Thomas coefficients of the (1, 4, 1) tridiagonal system, the same for every n
__device__ void spline_d2(const double* y, long st, int n, const double* __restrict__ cco, double* m) {
  for (int i = 0; i < n; ++i) m[i * st] = 0.0;
  if (n < 3) return;
  const int k = n - 2;
  double dp = 0.0;
  for (int i = 0; i < k; ++i) {
    const double r = 6.0 * (y[(i + 2) * st] - 2.0 * y[(i + 1) * st] + y[i * st]);
    const double d = i == 0 ? r * 0.25 : (r - dp) * cco[i];
    m[(i + 1) * st] = d;
    dp = d;
  }
  for (int i = k - 2; i >= 0; --i) m[(i + 1) * st] = m[(i + 1) * st] - cco[i] * m[(i + 2) * st];
}

__device__ __forceinline__ double spline_eval(const double* y, const double* m, long st, int n, double u) {
  if (n == 1) return y[0];
  const double fk = fmin(fmax(floor(u), 0.0), (double)(n - 2));
  const int k = (int)fk;
  const double t = u - fk, a = 1.0 - t;
  return a * y[k * st] + t * y[(k + 1) * st] + (a * a * a - a) * m[k * st] / 6.0 +
         (t * t * t - t) * m[(k + 1) * st] / 6.0;
}

// per field: median-filtered mesh grids (fb, fr), globalrms, second derivatives along the mesh rows (d2b, d2r).
// WEIGHTED (7z): before the median filter a bad mesh (NaN) takes, for background and rms separately, the mean of the good
// meshes of its field at the smallest squared distance, the tied ones added in raster order; the filled grids stand in d2b /
// d2r until the splines overwrite them.  nbad = the field's bad meshes; a field without a good mesh keeps NaN everywhere.
template <bool WEIGHTED>
__global__ __launch_bounds__(DT) void bkg_grid_kernel(const double* __restrict__ mback, const double* __restrict__ mrms,
                                                      int ny, int nx, int fs, const double* __restrict__ cco,
                                                      double* fb, double* fr, double* d2b, double* d2r,
                                                      double* __restrict__ grms, int* __restrict__ nbad) {
  __shared__ double s_red[4];
  __shared__ int s_w[4];
  const int tid = threadIdx.x;
  const int per = ny * nx;
  const long base = (long)blockIdx.x * per;
  const int h = fs / 2;
  if constexpr (WEIGHTED) {
    int bad = 0;
    for (int mi = tid; mi < per; mi += DT) {
      double b = mback[base + mi], r = mrms[base + mi];
      if (b != b) {
        ++bad;
        const int i = mi / nx, j = mi - (mi / nx) * nx;
        long best = -1;
        for (int q = 0; q < per; ++q) {
          if (mback[base + q] != mback[base + q]) continue;
          const long di = q / nx - i, dj = q - (q / nx) * nx - j, d = di * di + dj * dj;
          if (best < 0 || d < best) best = d;
        }
        double sb = 0.0, sr = 0.0;
        int cnt = 0;
        for (int q = 0; q < per && best >= 0; ++q) {
          if (mback[base + q] != mback[base + q]) continue;
          const long di = q / nx - i, dj = q - (q / nx) * nx - j;
          if (di * di + dj * dj != best) continue;
          sb += mback[base + q];
          sr += mrms[base + q];
          ++cnt;
        }
        b = best >= 0 ? sb / cnt : NAN;
        r = best >= 0 ? sr / cnt : NAN;
      }
      d2b[base + mi] = b;
      d2r[base + mi] = r;
    }
    bad = blk_isum(bad, s_w);
    if (tid == 0) nbad[blockIdx.x] = bad;
    __syncthreads();
  }
  for (int e = tid; e < 2 * per; e += DT) {
    const int which = e / per, mi = e - which * per, i = mi / nx, j = mi - (mi / nx) * nx;
    const double* g = (WEIGHTED ? (which ? d2r : d2b) : (which ? mrms : mback)) + base;
    double w[MF_MAX * MF_MAX];
    int n = 0;
    for (int a = max(0, i - h); a <= min(ny - 1, i + h); ++a)
      for (int b = max(0, j - h); b <= min(nx - 1, j + h); ++b) {
        const double x = g[a * nx + b];
        int q = n++;
        while (q > 0 && w[q - 1] > x) { w[q] = w[q - 1]; --q; }
        w[q] = x;
      }
    (which ? fr : fb)[base + mi] = median_sorted(w, n);
  }
  __syncthreads();
  double a[1] = {0.0};
  for (int e = tid; e < per; e += DT) a[0] += fr[base + e];
  blk_sum<1>(a, s_red);
  if (tid == 0) grms[blockIdx.x] = a[0] / per;
  for (int e = tid; e < 2 * nx; e += DT) {
    const int which = e / nx, j = e - which * nx;
    spline_d2((which ? fr : fb) + base + j, nx, ny, cco, (which ? d2r : d2b) + base + j);
  }
}

// one thread per (field, pixel row): the mesh-row splines at the row (g) and their spline along the columns (g2)
__global__ __launch_bounds__(DT) void bkg_row_kernel(const double* __restrict__ fb, const double* __restrict__ fr,
                                                     const double* __restrict__ d2b, const double* __restrict__ d2r,
                                                     int M, int H, int ny, int nx, int bs, int want_rms,
                                                     const double* __restrict__ cco, double* gb, double* gb2,
                                                     double* gr, double* gr2) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= (long)M * H) return;
  const long f = e / H;
  const int r = (int)(e - f * H);
  const double u = (r + 0.5) / bs - 0.5;
  const long gbase = f * (long)ny * nx;
  for (int which = 0; which < 1 + want_rms; ++which) {
    const double* y = (which ? fr : fb) + gbase;
    const double* m = (which ? d2r : d2b) + gbase;
    double* g = (which ? gr : gb) + e * nx;
    double* g2 = (which ? gr2 : gb2) + e * nx;
    for (int j = 0; j < nx; ++j) g[j] = spline_eval(y + j, m + j, nx, ny, u);
    spline_d2(g, 1, nx, cco, g2);
  }
}

// WEIGHTED (7z): v = 0 where the pixel does not count (a select: the value under the mask reaches nothing)
template <bool WEIGHTED>
__global__ __launch_bounds__(DT) void bkg_pixel_kernel(const double* __restrict__ data, const double* __restrict__ wt,
                                                       long total, int W, int nx,
                                                       int bs, const double* __restrict__ gb, const double* __restrict__ gb2,
                                                       const double* __restrict__ gr, const double* __restrict__ gr2,
                                                       double* __restrict__ v, double* __restrict__ back,
                                                       double* __restrict__ rms) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const long row = e / W;                         // field * H + pixel row
  const int c = (int)(e - row * W);
  const double u = (c + 0.5) / bs - 0.5;
  const double b = spline_eval(gb + row * nx, gb2 + row * nx, 1, nx, u);
  if constexpr (WEIGHTED) v[e] = counts(wt[e]) ? data[e] - b : 0.0;
  else v[e] = data[e] - b;
  if (back) back[e] = b;
  if (rms) rms[e] = spline_eval(gr + row * nx, gr2 + row * nx, 1, nx, u);
}

// Multi-band detection (7za): one thread per pixel, the k selected bands in an inner loop; plane f * k + j is band j of field
// f in data, pl (the planes P, PLANES only), the row splines and bgrms.  Per band the two splines as bkg_pixel_kernel
// evaluates them, v_j = data_j - back_j, w_j = 1 / rms^2 | P / rms^2 | P (ABSOLUTE); the band counts iff 0 < w_j < inf, with
// planes also 0 < P_j < inf, and it has a good mesh in the field (bgrms not NaN).  num = sum (c_j w_j) v_j and
// Wt = sum (c_j c_j) w_j over the counting bands in scalar accumulators, V = 0 | v_j / c_j | num / Wt for 0 | 1 | more of
// them.  A value under a band that does not count is not read.  back / rms [..][k] only when the caller wants the maps; with
// ABSOLUTE and no rms map the rms splines are not evaluated (bkg_row_kernel did not make them).
template <bool PLANES, bool ABSOLUTE>
__global__ __launch_bounds__(DT) void multiband_pixel_kernel(const double* __restrict__ data, const double* __restrict__ pl,
                                                             long total, int H, int W, int k, int nx, int bs,
                                                             const double* __restrict__ gb, const double* __restrict__ gb2,
                                                             const double* __restrict__ gr, const double* __restrict__ gr2,
                                                             const double* __restrict__ bgrms, const double* __restrict__ cw,
                                                             double* __restrict__ V, double* __restrict__ Wt,
                                                             double* __restrict__ back, double* __restrict__ rms) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const long HW = (long)H * W;
  const long f = e / HW;
  const long p = e - f * HW;
  const int r = (int)(p / W), c = (int)(p - (long)r * W);
  const double u = (c + 0.5) / bs - 0.5;
  const bool need_rms = !ABSOLUTE || rms != nullptr;
  double num = 0.0, wsum = 0.0, v1 = 0.0, c1 = 1.0;
  int n = 0;
  for (int j = 0; j < k; ++j) {
    const long plane = f * k + j;
    const long row = plane * H + r;
    const double b = spline_eval(gb + row * nx, gb2 + row * nx, 1, nx, u);
    const double sg = need_rms ? spline_eval(gr + row * nx, gr2 + row * nx, 1, nx, u) : 0.0;
    if (back) back[e * k + j] = b;
    if (rms) rms[e * k + j] = sg;
    const double P = PLANES ? pl[plane * HW + p] : 1.0;
    const double w = ABSOLUTE ? P : P / (sg * sg);
    const double g = bgrms[plane];
    if (g == g && counts(w) && (!PLANES || counts(P))) {
      const double cj = cw[j];
      const double v = data[plane * HW + p] - b;
      num += (cj * w) * v;
      wsum += (cj * cj) * w;
      v1 = v;
      c1 = cj;
      ++n;
    }
  }
  V[e] = n == 0 ? 0.0 : (n == 1 ? v1 / c1 : num / wsum);
  Wt[e] = n == 0 ? 0.0 : wsum;
}

// (7za) the diagnostic globalrms of the combination per field, 1 / sqrt(sum (c_j c_j) / (g_j g_j)) over the bands with a good
// mesh, j ascending; NaN for a field without one (filter_kernel then puts nothing above the threshold)
__global__ __launch_bounds__(DT) void multiband_grms_kernel(const double* __restrict__ bgrms, const double* __restrict__ cw,
                                                            int m, int k, double* __restrict__ fgrms) {
  const int f = blockIdx.x * DT + threadIdx.x;
  if (f >= m) return;
  double acc = 0.0;
  bool any = false;
  for (int j = 0; j < k; ++j) {
    const double g = bgrms[(long)f * k + j];
    if (g == g) {
      acc += (cw[j] * cw[j]) / (g * g);
      any = true;
    }
  }
  fgrms[f] = any ? 1.0 / sqrt(acc) : NAN;
}

// D = correlation of v with kn (normalised taps), zero outside the field; par = own index where D > T, T = thresh * globalrms
// or (absolute) thresh.  WEIGHTED (7z): D holds the significance S.  A second tile holds w, zero where the pixel does not
// count and outside the field; conv: S = (sum kn v) sqrt(w); MATCHED: the first tile holds v w and
// S = (sum kn (v w)) / sqrt(sum (kn kn) w), -inf where the denominator is 0; S = -inf at a pixel that does not count, and
// nothing is above the threshold in a field without a good mesh (globalrms NaN).
template <bool WEIGHTED, bool MATCHED>
__global__ __launch_bounds__(DT) void filter_kernel(const double* __restrict__ v, const double* __restrict__ wt, int H, int W,
                                                    const double* __restrict__ kn, int kh, int kw,
                                                    const double* __restrict__ grms, double thresh, int absolute,
                                                    double* __restrict__ D, int* __restrict__ par) {
  __shared__ double t[(FT + KMAX - 1) * (FT + KMAX - 1)];
  __shared__ double tw[WEIGHTED ? (FT + KMAX - 1) * (FT + KMAX - 1) : 1];
  const int tid = threadIdx.x;
  const long f = blockIdx.z;
  const int r0 = blockIdx.y * FT, c0 = blockIdx.x * FT, ry = kh / 2, rx = kw / 2;
  const int TH = FT + kh - 1, TW = FT + kw - 1;
  const long fb = f * (long)H * W;
  for (int e = tid; e < TH * TW; e += DT) {
    const int a = e / TW, b = e - (e / TW) * TW, r = r0 - ry + a, c = c0 - rx + b;
    const bool in = r >= 0 && r < H && c >= 0 && c < W;
    if constexpr (WEIGHTED) {
      const double w = in ? wt[fb + (long)r * W + c] : 0.0;
      const bool on = counts(w);
      const double x = on ? v[fb + (long)r * W + c] : 0.0;
      tw[e] = on ? w : 0.0;
      t[e] = MATCHED ? (on ? x * w : 0.0) : x;
    } else {
      t[e] = in ? v[fb + (long)r * W + c] : 0.0;
    }
  }
  __syncthreads();
  const int ty = tid / FT, tx = tid % FT, r = r0 + ty, c = c0 + tx;
  if (r >= H || c >= W) return;
  double acc = 0.0, den = 0.0;
  for (int a = 0; a < kh; ++a)
    for (int b = 0; b < kw; ++b) {
      const double k = kn[a * kw + b];
      acc += k * t[(ty + a) * TW + tx + b];
      if constexpr (WEIGHTED && MATCHED) den += (k * k) * tw[(ty + a) * TW + tx + b];
    }
  const long o = fb + (long)r * W + c;
  if constexpr (WEIGHTED) {
    const double wc = tw[(ty + ry) * TW + tx + rx];
    if (MATCHED) acc = (wc > 0.0 && den > 0.0) ? acc / sqrt(den) : -INFINITY;
    else acc = wc > 0.0 ? acc * sqrt(wc) : -INFINITY;
    const double g = grms[f];
    const double T = absolute ? thresh : thresh * g;
    D[o] = acc;
    par[o] = (g == g && acc > T) ? r * W + c : -1;
  } else {
    D[o] = acc;
    par[o] = acc > thresh * grms[f] ? r * W + c : -1;
  }
}

// ---- connected components ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT) void cc_merge_kernel(int* par, long total, int W, long HW) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const long f = e / HW;
  const int p = (int)(e - f * HW), r = p / W, c = p - (p / W) * W;
  int* P = par + f * HW;
  if (ald(P + p) < 0) return;
  if (c > 0 && ald(P + p - 1) >= 0) uf_union(P, p, p - 1);
  if (r > 0) {
    const int q = p - W;
    if (c > 0 && ald(P + q - 1) >= 0) uf_union(P, p, q - 1);
    if (ald(P + q) >= 0) uf_union(P, p, q);
    if (c + 1 < W && ald(P + q + 1) >= 0) uf_union(P, p, q + 1);
  }
}

// label = root (smallest raster index of the component) or -1; area and bounding box per root
__global__ __launch_bounds__(DT) void cc_flatten_kernel(int* par, long total, int W, long HW, int* __restrict__ lab,
                                                        int* area, int* cmin, int* cmax, int* rmax) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const long f = e / HW;
  const int p = (int)(e - f * HW);
  int* P = par + f * HW;
  if (ald(P + p) < 0) { lab[e] = -1; return; }
  const int rt = uf_find(P, p);
  lab[e] = rt;
  const long o = f * HW + rt;
  aadd(area + o, 1);
  const int r = p / W, c = p - (p / W) * W;
  (void)__hip_atomic_fetch_min(cmin + o, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(cmax + o, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(rmax + o, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int CC_PER = 16;                        // consecutive pixels per thread in the compaction scan

// per field: the components of >= minarea pixels in root order -> table [ccap][5] = root, area, cmin, cmax, rmax
__global__ __launch_bounds__(DT) void cc_compact_kernel(const int* __restrict__ lab, const int* __restrict__ area,
                                                        const int* __restrict__ cmin, const int* __restrict__ cmax,
                                                        const int* __restrict__ rmax, long HW, int minarea, long ccap,
                                                        int* __restrict__ table, int* __restrict__ ncomp) {
  __shared__ int s_w[4];
  const long fb = (long)blockIdx.x * HW;
  int* tab = table + (long)blockIdx.x * ccap * 5;
  int count = 0;
  for (long base = 0; base < HW; base += (long)DT * CC_PER) {
    const long p0 = base + (long)threadIdx.x * CC_PER;
    int mine = 0;
    for (int q = 0; q < CC_PER; ++q) {
      const long p = p0 + q;
      if (p < HW && lab[fb + p] == (int)p && area[fb + p] >= minarea) ++mine;
    }
    int tot;
    int at = count + blk_scan(mine, s_w, tot);
    for (int q = 0; q < CC_PER && mine > 0; ++q) {
      const long p = p0 + q;
      if (p < HW && lab[fb + p] == (int)p && area[fb + p] >= minarea) {
        int* row = tab + (long)at * 5;
        row[0] = (int)p;
        row[1] = area[fb + p];
        row[2] = cmin[fb + p];
        row[3] = cmax[fb + p];
        row[4] = rmax[fb + p];
        ++at;
        --mine;
      }
    }
    count += tot;
  }
  if (threadIdx.x == 0) ncomp[blockIdx.x] = count;
}

// labels map of the API: the component's root for the pixels of components of >= minarea pixels, -1 elsewhere
__global__ __launch_bounds__(DT) void cc_labels_kernel(const int* __restrict__ lab, const int* __restrict__ area, long total,
                                                       long HW, int minarea, int* __restrict__ out) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const int l = lab[e];
  out[e] = (l >= 0 && area[e - e % HW + l] >= minarea) ? l : -1;
}

// ---- deblending -------------------------------------------------------------------------------------------------
// (7zb) seg holds 0 outside every object and the object's rank in its component + 1 inside, job the component's job there:
// base[j] = the objects of the earlier components of the job's field
__global__ __launch_bounds__(DT) void seg_base_kernel(int* __restrict__ seg, const int* __restrict__ job,
                                                      const int* __restrict__ base, long total) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= total) return;
  const int v = seg[e];
  if (v > 0) seg[e] = v + base[job[e]];
}

inline unsigned nblk(long total) { return (unsigned)((total + DT - 1) / DT); }

// device bytes one H x W field can need in a launch: deblend scratch and catalog slots sized as if every pixel lay in
// a component
// (7za) k > 0: k data planes, k planes of P when given, k x the mesh grids and row splines, the combined weight Wt, and for a
// host source the interleaved staging lines of max(nb, k) values per pixel
// (7zb) objects: the slots of the new columns and every job's segmap base; segmap: 4 bytes per pixel
// (7zc) clean: the tables of CleanTables per raw object (at most HW / minarea of them in a field) and per field
// DetectMode: what a call runs, derived once from its request; every stage, field_bytes and DetectWork::alloc read it.
// DetectGeom: H x W pixel fields on ny x nx background meshes, HW pixels and at most ccap components of >= minarea pixels each.
struct DetectMode {
  bool dev;                        // the fields lie in device memory (nwhich field numbers, 0 for a host source)
  int nwhich;
  bool weighted;                   // (7z) single-band weights
  int k;                           // (7za) the selected bands, 0: one band
  bool planes, planes_abs;         // (7za) planes are given; and their noise is absolute
  int nb_src, stage_nb;            // bands of the source; values per pixel of a host multi-band source's staging lines
  bool absolute, matched;          // T = thresh, not thresh * globalrms; the matched filter
  bool objects, segmap;            // (7zb) the object columns; and the segmap
  bool clean;                      // (7zc) the cleaning pass: objects and segmap are then on, whatever the caller asks for
  bool back, rms, labels, maps;    // the maps asked for; maps: any of back, rms, D, labels
  bool multi() const { return k > 0; }
  bool wplanes() const { return weighted || planes; }    // the WEIGHTED background kernels run: wt and nbad exist
  int kk() const { return k > 0 ? k : 1; }               // planes per field
};
struct DetectGeom { int H, W, ny, nx; long HW, ccap; };

// (7zc) ints rfield rbox[4] rnum rnpix absorber root[2] rootout newrow, doubles rd[6] mthresh der[6]; fptr nsurv, T
constexpr long CLEAN_ROW_INTS = 12, CLEAN_ROW_DOUBLES = 13, CLEAN_ROW_BYTES = CLEAN_ROW_INTS * 4 + CLEAN_ROW_DOUBLES * 8;
constexpr long CLEAN_FIELD_BYTES = 2 * 4 + 4 + 8;
constexpr int CLEAN_MINAREA_MAX = 64;

long field_bytes(const DetectGeom& g, const DetectMode& md) {
  const long H = g.H, HW = g.HW, ny = g.ny, nx = g.nx, capn = g.ccap, k = md.k;
  long b = HW * (8 + 8 + 8 + 4 * 7);                          // data v D | par lab area cmin cmax rmax lidx
  if (md.maps) b += HW * (8 + 8 + 4);                         // back rms labels
  if (md.weighted) b += HW * 8 + 4;                           // the weight plane, the bad-mesh count
  if (k > 0) {
    b += HW * 8 * (k - 1) + HW * 8 + (md.planes ? HW * 8 * k : 0) + HW * 8 * md.stage_nb;
    if (md.maps) b += HW * (8 + 8) * (k - 1);
    b += (k - 1) * (H * nx * 4 * 8 + ny * nx * 6 * 8) + k * (8 + 4) + 8;   // ... band globalrms, bad meshes, globalrms
  }
  b += H * nx * 4 * 8 + ny * nx * 6 * 8;                      // row splines, mesh grids
  b += capn * 5 * 4;                                          // component table
  b += HW * (8 + 6 * 4) + capn * ((2 + OBJ_D) * 8 + 3 * 4);   // deblend scratch
  b += capn * ((long)sizeof(DbJob) + 4 * 4 + 4 * 8);          // jobs and catalog slots
  if (md.objects) b += capn * (OBJ_I * 4 + DET_OBJ_D * 8 + 4);
  if (md.segmap) b += HW * 4;
  if (md.clean) b += capn * CLEAN_ROW_BYTES + CLEAN_FIELD_BYTES;
  return b;
}

// data[i] = band `band` of field which[i] of a stack of [HW][nb] fields: the contiguous planes the detector kernels read
__global__ __launch_bounds__(DT) void band_gather_kernel(const double* __restrict__ fields, long HW, int nb, int band,
                                                         const int* __restrict__ which, double* __restrict__ data) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= HW) return;
  const long f = which[blockIdx.y];
  data[(long)blockIdx.y * HW + e] = fields[(f * HW + e) * nb + band];
}

// (7za) plane blockIdx.y * k + j of data = band bands[j] of field which[blockIdx.y] (null: blockIdx.y itself) of a stack of
// [HW][nb] fields: one pass in which every pixel's line is read once, for the k selected bands
__global__ __launch_bounds__(DT) void bands_gather_kernel(const double* __restrict__ fields, long HW, int nb,
                                                          const int* __restrict__ bands, int k, const int* __restrict__ which,
                                                          double* __restrict__ data) {
  const long e = (long)blockIdx.x * DT + threadIdx.x;
  if (e >= HW) return;
  const long f = which ? which[blockIdx.y] : blockIdx.y;
  const double* line = fields + (f * HW + e) * nb;
  for (int j = 0; j < k; ++j) data[((long)blockIdx.y * k + j) * HW + e] = line[bands[j]];
}

// the device buffers of scene_detect.  DetectWork: the workspace of one launch's fields (chunk fields of H x W pixels on
// ny x nx background meshes); back / rms / labout exist only when the caller wants those maps, wdev (the nwhich field numbers
// of a device source) only when the fields come from device memory.
struct DetectWork {
  DevBuf<double> data, v, D, mb, mr, fbk, frm, d2b, d2r, gb, gb2, gr, gr2, grms, kdev, cdev, back, rms, wt;
  DevBuf<int> par, lab, area, cmin, cmax, rmax, lidx, table, ncomp, labout, wdev, nbad;
  // (7za) bands > 0: everything per band (data, wt, the mesh grids, the row splines, grms, nbad, the back / rms maps) holds
  // bands planes per field, plane f * bands + j; cw = Wt, fgrms = the fields' globalrms, stage = the interleaved lines of a
  // host source, bsel = the band numbers then 0 .. bands - 1, cband = the c_j
  DevBuf<double> cw, fgrms, stage, cband;
  DevBuf<int> bsel;
  DevBuf<int> seg;                                   // (7zb) the launch's segmap, when asked for
  int alloc(int chunk, const DetectGeom& g, const DetectMode& md, size_t ktaps, size_t ccoef) {
    if (md.segmap) DV_TRY(seg.alloc((size_t)chunk * g.H * g.W));
    const size_t kk = (size_t)md.kk();
    const size_t px = (size_t)chunk * g.H * g.W, grid = kk * chunk * g.ny * g.nx, rows = kk * chunk * g.H * g.nx;
    DV_TRY(data.alloc(kk * px));
    for (DevBuf<double>* b : {&v, &D}) DV_TRY(b->alloc(px));
    for (DevBuf<int>* b : {&par, &lab, &area, &cmin, &cmax, &rmax, &lidx}) DV_TRY(b->alloc(px));
    for (DevBuf<double>* b : {&mb, &mr, &fbk, &frm, &d2b, &d2r}) DV_TRY(b->alloc(grid));
    for (DevBuf<double>* b : {&gb, &gb2, &gr, &gr2}) DV_TRY(b->alloc(rows));
    DV_TRY(grms.alloc(kk * chunk)); DV_TRY(ncomp.alloc((size_t)chunk)); DV_TRY(table.alloc((size_t)chunk * g.ccap * 5));
    DV_TRY(kdev.alloc(ktaps)); DV_TRY(cdev.alloc(ccoef));
    if (md.back) DV_TRY(back.alloc(kk * px));
    if (md.rms) DV_TRY(rms.alloc(kk * px));
    if (md.labels) DV_TRY(labout.alloc(px));
    if (md.nwhich > 0) DV_TRY(wdev.alloc((size_t)md.nwhich));
    if (md.wplanes()) { DV_TRY(wt.alloc(kk * px)); DV_TRY(nbad.alloc(kk * chunk)); }   // (7z) the weight planes, the bad meshes
    if (md.multi()) {
      DV_TRY(cw.alloc(px)); DV_TRY(fgrms.alloc((size_t)chunk)); DV_TRY(bsel.alloc(2 * kk)); DV_TRY(cband.alloc(kk));
      if (md.stage_nb > 0) DV_TRY(stage.alloc(px * md.stage_nb));
    }
    return OK;
  }
};
// DeblendScratch: the jobs of one launch's components, their scratch and their catalogue slots, sized once the components
// are known and freed before the next launch sizes its own
struct DeblendScratch {
  DevBuf<DbJob> djobs;
  DevBuf<double> dscr, o_peak, o_flux, o_x, o_y;
  DevBuf<int> iscr, nobj, o_npix, o_pp;
  DevBuf<int> oi, jbase;                             // (7zb) [slots][OBJ_I], [nj]; od [slots][DET_OBJ_D]
  DevBuf<double> od;
  int alloc(long nj, long dws, long iws, long slots, bool objects = false) {
    if (objects) {
      DV_TRY(oi.alloc((size_t)slots * OBJ_I)); DV_TRY(od.alloc((size_t)slots * DET_OBJ_D)); DV_TRY(jbase.alloc((size_t)nj));
    }
    DV_TRY(djobs.alloc((size_t)nj + (objects ? 1 : 0))); DV_TRY(nobj.alloc((size_t)nj));
    DV_TRY(dscr.alloc((size_t)dws)); DV_TRY(iscr.alloc((size_t)iws));
    for (DevBuf<int>* b : {&o_npix, &o_pp}) DV_TRY(b->alloc((size_t)slots));
    for (DevBuf<double>* b : {&o_peak, &o_flux, &o_x, &o_y}) DV_TRY(b->alloc((size_t)slots));
    return OK;
  }
};

// ---- the host path: the checks, the mode, and one call's stages (DetectRun) in the order they run --------------------
// 1. the argument checks, before any GPU work, in the order the refusals have always had
int detect_check(const DetectRequest& rq) {
  const DetectDevSrc* dev = rq.dev;
  const DetectWeights* wq = rq.weights;
  const DetectBands* mb = rq.bands;
  const DetectCatalog& c = rq.cat;
  if (dev && (!dev->fields_dev || !dev->which_h || dev->nb < 1 || dev->band < 0 || dev->band >= dev->nb)) {
    set_error("scene_detect: bad device source");
    return E_INVALID;
  }
  const dv_detect_params* p = rq.par;
  if (!p || (!rq.fields_h && !dev) || rq.M < 0 || rq.H < 1 || rq.W < 1 || rq.H > DIM_MAX || rq.W > DIM_MAX ||
      (long)rq.H * rq.W > 0x7fffffffL || !std::isfinite(p->thresh) || !std::isfinite(p->cont) || p->minarea < 1 ||
      p->nthresh < 1 || p->nthresh > 1024 || p->back_size < 1 || p->back_size > 64 || p->back_filter < 1 ||
      p->back_filter > MF_MAX || (p->back_filter & 1) == 0 || c.cap < 0 || !c.n_out || !c.offsets_h || !c.globalrms_h ||
      p->workspace_bytes < 0 ||
      (c.cap > 0 && (!c.field_h || !c.parent_h || !c.npix_h || !c.peak_h || !c.flux_h || !c.x_h || !c.y_h))) {
    set_error("scene_detect: bad arguments");
    return E_INVALID;
  }
  if ((rq.objects || rq.clean) && p->thresh < 0.0) {    // (7zb) the moments' weights D > T must be positive
    set_error("scene_detect: the object shapes and the segmap need thresh >= 0 (got %g)", p->thresh);
    return E_INVALID;
  }
  if (rq.clean) {                                       // (7zc)
    const double beta = rq.clean->clean_param;
    if (!std::isfinite(beta) || !(beta > 0.0)) {
      set_error("scene_detect: clean_param must be finite and > 0 (got %g)", beta);
      return E_INVALID;
    }
    if (!(p->thresh > 0.0)) {
      set_error("scene_detect: the cleaning pass compares profiles with the threshold, thresh must be > 0 (got %g)", p->thresh);
      return E_INVALID;
    }
    if (p->minarea > CLEAN_MINAREA_MAX) {
      set_error("scene_detect: the cleaning pass takes minarea up to %d (got %d)", CLEAN_MINAREA_MAX, p->minarea);
      return E_INVALID;
    }
  }
  if (mb) {
    if (wq) {
      set_error("scene_detect: single-band weights and a band selection exclude each other");
      return E_INVALID;
    }
    DV_TRY(detect_bands_check("scene_detect_multiband", mb->bands, mb->k, mb->c, dev ? dev->nb : rq.nb,
                              mb->has_planes ? mb->noise : 0, mb->filter));
    if (mb->has_planes && (dev ? !dev->planes_dev : !mb->planes_h)) {
      set_error("scene_detect_multiband: planes announced but not given");
      return E_INVALID;
    }
    if (!(p->thresh > 0.0)) {
      set_error("scene_detect_multiband: the threshold is in units of the combined pixel's sigma and must be > 0 (got %g)",
                p->thresh);
      return E_INVALID;
    }
  }
  if (wq) {
    if (dev ? !dev->weights_dev : !wq->weights_h) {
      set_error("scene_detect: weighted detection without weights");
      return E_INVALID;
    }
    if ((wq->noise != 0 && wq->noise != 1) || (wq->filter != 0 && wq->filter != 1)) {
      set_error("scene_detect: noise must be 0 (absolute) or 1 (relative) and filter 0 (conv) or 1 (matched), got %d, %d",
                wq->noise, wq->filter);
      return E_INVALID;
    }
    if (wq->noise == 0 && !(p->thresh > 0.0)) {
      set_error("scene_detect: with absolute noise the threshold is in units of sigma and must be > 0 (got %g)", p->thresh);
      return E_INVALID;
    }
  }
  if (p->kernel && (p->kh < 1 || p->kw < 1 || p->kh > KMAX || p->kw > KMAX || (p->kh & 1) == 0 || (p->kw & 1) == 0)) {
    set_error("scene_detect: the filter kernel must have odd sizes of 1 .. %d (got %d x %d)", KMAX, p->kh, p->kw);
    return E_INVALID;
  }
  return OK;
}

// the mode of a checked request (with bands the weights are null and the fields interleaved)
DetectMode detect_mode(const DetectRequest& rq) {
  const DetectWeights* wq = rq.weights;
  const DetectBands* mb = rq.bands;
  DetectMode md{};
  md.dev = rq.dev != nullptr; md.nwhich = rq.dev ? rq.M : 0;
  md.weighted = wq != nullptr;
  md.k = mb ? mb->k : 0; md.planes = mb && mb->has_planes; md.planes_abs = md.planes && mb->noise == 0;
  md.nb_src = rq.dev ? rq.dev->nb : rq.nb; md.stage_nb = (mb && !rq.dev) ? std::max(md.nb_src, md.k) : 0;
  md.absolute = mb || (wq && wq->noise == 0); md.matched = mb ? mb->filter == 1 : (wq && wq->filter == 1);
  md.clean = rq.clean != nullptr;
  md.objects = rq.objects || md.clean; md.segmap = (rq.objects && rq.objects->segmap_h) || md.clean;
  md.back = rq.back_h != nullptr; md.rms = rq.rms_h != nullptr; md.labels = rq.labels_h != nullptr;
  md.maps = rq.back_h || rq.rms_h || rq.D_h || rq.labels_h;
  return md;
}

// 2. the filter taps divided by sum |k|; the default is the pixel-integrated circular Gaussian of DESIGN 7e
struct DetectTaps { std::vector<double> kn; int kh, kw; };
int detect_taps(const dv_detect_params& p, DetectTaps& t) {
  if (p.kernel) {
    t.kh = p.kh; t.kw = p.kw;
    t.kn.assign(p.kernel, p.kernel + (size_t)p.kh * p.kw);
  } else {
    t.kh = t.kw = 7;
    const double sq = std::sqrt(2.0) * 1.27627;
    double g[7];
    for (int a = 0; a < 7; ++a) g[a] = std::erf((a - 3 + 0.5) / sq) - std::erf((a - 3 - 0.5) / sq);
    t.kn.resize(49);
    for (int a = 0; a < 7; ++a)
      for (int b = 0; b < 7; ++b) t.kn[a * 7 + b] = g[a] * g[b];
  }
  double ksum = 0.0;
  for (double k : t.kn) ksum += std::fabs(k);
  if (!(ksum > 0.0) || !std::isfinite(ksum)) {
    set_error("scene_detect: the filter kernel has no finite non-zero tap");
    return E_INVALID;
  }
  for (double& k : t.kn) k /= ksum;
  return OK;
}

// one launch: the fields f0 .. f0 + m of the call, px pixels, mk planes
struct DetectLaunch { int f0, m; long px; int mk; };
// its components as the deblender takes them: a job each with its scratch and catalogue slots placed, jfield the job's field
// in the call, and the totals
struct DetectJobs { std::vector<DbJob> jobs; std::vector<int> jfield; long nj = 0, dws = 0, iws = 0, slots = 0; };
// what the deblender wrote, on the host: objects per job, the columns per catalogue slot (oi, od: the rows of 7zb); and as
// HostCatalog the catalogue of all fields of the call, grown launch by launch (oi, od: rows of DET_OBJ_I ints, DET_OBJ_D doubles)
struct DetectSlots { std::vector<int> nobj, npix, oi; std::vector<double> peak, flux, x, y, od; };
struct HostCatalog {
  std::vector<int32_t> field, parent, npix, oi, nmerged; std::vector<double> peak, flux, x, y, od, mthresh;
  void truncate(size_t n) {
    for (std::vector<int32_t>* v : {&field, &parent, &npix, &nmerged}) if (v->size() > n) v->resize(n);
    for (std::vector<double>* v : {&peak, &flux, &x, &y, &mthresh}) if (v->size() > n) v->resize(n);
    if (oi.size() > n * DET_OBJ_I) oi.resize(n * DET_OBJ_I);
    if (od.size() > n * DET_OBJ_D) od.resize(n * DET_OBJ_D);
  }
};
// (7zc) what the cleaning pass found, per raw object of the launch in catalogue order: its root (a raw object of the launch),
// the root's row among the survivors of its field, its mthresh; fptr: every field's first raw object
struct DetectCleaned { std::vector<int> root, newrow, fptr; std::vector<double> mthresh; };

// one call: the request, what it asks for, the device workspace and the catalogue so far; the stages are its methods
struct DetectRun {
  const DetectRequest& rq; const dv_detect_params& p; const DetectMode md; const DetectGeom g; const DetectTaps& taps;
  hipStream_t s;
  DetectWork w;
  std::vector<double> cco;
  std::vector<int> h_ncomp;
  HostCatalog cat;

  // what every launch reads, once: the workspace for `chunk` fields, the taps, the coefficients of the spline's tridiagonal
  // solve, a device source's field numbers, the band numbers (then 0 .. k - 1) and the c_j
  int prepare(int chunk) {
    h_ncomp.resize((size_t)std::max(chunk, 1));
    if (chunk == 0) return OK;
    cco.resize((size_t)std::max(g.ny, g.nx) + 1);
    cco[0] = 0.25;
    for (size_t i = 1; i < cco.size(); ++i) cco[i] = 1.0 / (4.0 - cco[i - 1]);
    DV_TRY(w.alloc(chunk, g, md, taps.kn.size(), cco.size()));
    DV_HIP(hipMemcpyAsync(w.kdev, taps.kn.data(), taps.kn.size() * sizeof(double), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(w.cdev, cco.data(), cco.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (md.dev) DV_HIP(hipMemcpyAsync(w.wdev, rq.dev->which_h, (size_t)rq.M * sizeof(int), hipMemcpyHostToDevice, s));
    if (md.multi()) {
      std::vector<int> sel((size_t)2 * md.k);
      std::vector<double> cb((size_t)md.k, 1.0);
      for (int j = 0; j < md.k; ++j) {
        sel[j] = rq.bands->bands[j];
        sel[md.k + j] = j;
        if (rq.bands->c) cb[j] = rq.bands->c[j];
      }
      DV_HIP(hipMemcpyAsync(w.bsel, sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice, s));
      DV_HIP(hipMemcpyAsync(w.cband, cb.data(), cb.size() * sizeof(double), hipMemcpyHostToDevice, s));
      DV_HIP(hipStreamSynchronize(s));                    // (sel and cb leave scope)
    }
    return OK;
  }

  // (7za) the md.k planes `sel` of the launch's lines of nb values at src -> dst; which: a device stack's field numbers
  int gather(const double* src, int nb, const int* sel, const int* which, double* dst, const DetectLaunch& L) {
    hipLaunchKernelGGL(bands_gather_kernel, dim3(nblk(g.HW), (unsigned)L.m), dim3(DT), 0, s, src, g.HW, nb, sel, md.k, which, dst);
    DV_HIP(hipGetLastError());
    return OK;
  }
  // 3. the launch's planes into w.data (and w.wt): uploaded, or gathered from the staged interleaved lines or the device stack
  int load_planes(const DetectLaunch& L) {
    const DetectDevSrc* dev = rq.dev;
    const size_t at = (size_t)L.f0 * g.HW, px = (size_t)L.px;
    const int* which = dev ? w.wdev + L.f0 : nullptr;
    if (md.multi()) {
      const size_t nb = (size_t)md.nb_src, k = (size_t)md.k;
      if (!dev) DV_HIP(hipMemcpyAsync(w.stage, rq.fields_h + at * nb, px * nb * sizeof(double), hipMemcpyHostToDevice, s));
      DV_TRY(gather(dev ? dev->fields_dev : w.stage.get(), md.nb_src, w.bsel, which, w.data, L));
      if (md.planes) {
        if (!dev) DV_HIP(hipMemcpyAsync(w.stage, rq.bands->planes_h + at * k, px * k * sizeof(double), hipMemcpyHostToDevice, s));
        DV_TRY(gather(dev ? dev->planes_dev : w.stage.get(), md.k, w.bsel + md.k, which, w.wt, L));
      }
    } else if (dev) {
      const dim3 grid(nblk(g.HW), (unsigned)L.m);
      hipLaunchKernelGGL(band_gather_kernel, grid, dim3(DT), 0, s, dev->fields_dev, g.HW, dev->nb, dev->band, which, w.data);
      DV_HIP(hipGetLastError());
      if (md.weighted) {
        hipLaunchKernelGGL(band_gather_kernel, grid, dim3(DT), 0, s, dev->weights_dev, g.HW, 1, 0, which, w.wt);
        DV_HIP(hipGetLastError());
      }
    } else {
      DV_HIP(hipMemcpyAsync(w.data, rq.fields_h + at, px * sizeof(double), hipMemcpyHostToDevice, s));
      if (md.weighted) DV_HIP(hipMemcpyAsync(w.wt, rq.weights->weights_h + at, px * sizeof(double), hipMemcpyHostToDevice, s));
    }
    return OK;
  }

  // 4. the background: meshes, grids and row splines per plane, then v per pixel - or (7za) V and Wt of the bands combined
  int background(const DetectLaunch& L) {
    const int H = g.H, W = g.W, ny = g.ny, nx = g.nx, bs = p.back_size, mk = L.mk;
    const long px = L.px;
    const dim3 gmesh((unsigned)((long)mk * ny * nx)), gpix(nblk(px)), blk(DT);
    if (md.wplanes()) {
      hipLaunchKernelGGL(bkg_mesh_kernel<true>, gmesh, blk, 0, s, w.data, w.wt, H, W, bs, ny, nx, w.mb, w.mr);
      DV_HIP(hipGetLastError());
      hipLaunchKernelGGL(bkg_grid_kernel<true>, dim3((unsigned)mk), blk, 0, s, w.mb, w.mr, ny, nx, p.back_filter, w.cdev, w.fbk,
                         w.frm, w.d2b, w.d2r, w.grms, w.nbad);
    } else {
      hipLaunchKernelGGL(bkg_mesh_kernel<false>, gmesh, blk, 0, s, w.data, nullptr, H, W, bs, ny, nx, w.mb, w.mr);
      DV_HIP(hipGetLastError());
      hipLaunchKernelGGL(bkg_grid_kernel<false>, dim3((unsigned)mk), blk, 0, s, w.mb, w.mr, ny, nx, p.back_filter, w.cdev, w.fbk,
                         w.frm, w.d2b, w.d2r, w.grms, nullptr);
    }
    DV_HIP(hipGetLastError());
    hipLaunchKernelGGL(bkg_row_kernel, dim3(nblk((long)mk * H)), blk, 0, s, w.fbk, w.frm, w.d2b, w.d2r, mk, H, ny, nx, bs,
                       (md.rms || (md.multi() && !md.planes_abs)) ? 1 : 0, w.cdev, w.gb, w.gb2, w.gr, w.gr2);
    DV_HIP(hipGetLastError());
    if (md.multi()) {
      hipLaunchKernelGGL(multiband_grms_kernel, dim3(nblk(L.m)), blk, 0, s, w.grms, w.cband, L.m, md.k, w.fgrms);
      DV_HIP(hipGetLastError());
      if (md.planes_abs)
        hipLaunchKernelGGL((multiband_pixel_kernel<true, true>), gpix, blk, 0, s, w.data, w.wt, px, H, W, md.k, nx, bs, w.gb,
                           w.gb2, w.gr, w.gr2, w.grms, w.cband, w.v, w.cw, w.back, w.rms);
      else if (md.planes)
        hipLaunchKernelGGL((multiband_pixel_kernel<true, false>), gpix, blk, 0, s, w.data, w.wt, px, H, W, md.k, nx, bs, w.gb,
                           w.gb2, w.gr, w.gr2, w.grms, w.cband, w.v, w.cw, w.back, w.rms);
      else
        hipLaunchKernelGGL((multiband_pixel_kernel<false, false>), gpix, blk, 0, s, w.data, nullptr, px, H, W, md.k, nx, bs, w.gb,
                           w.gb2, w.gr, w.gr2, w.grms, w.cband, w.v, w.cw, w.back, w.rms);
    } else if (md.weighted)
      hipLaunchKernelGGL(bkg_pixel_kernel<true>, gpix, blk, 0, s, w.data, w.wt, px, W, nx, bs, w.gb, w.gb2, w.gr, w.gr2, w.v,
                         w.back, w.rms);
    else
      hipLaunchKernelGGL(bkg_pixel_kernel<false>, gpix, blk, 0, s, w.data, nullptr, px, W, nx, bs, w.gb, w.gb2, w.gr, w.gr2, w.v,
                         w.back, w.rms);
    DV_HIP(hipGetLastError());
    return OK;
  }

  // 5. D (with weights the significance S) and the segmentation's initial parents; (7za) V, Wt and the combined globalrms
  // stand where v, w and globalrms stand, with absolute noise
  int filter(const DetectLaunch& L) {
    const dim3 grid((unsigned)((g.W + FT - 1) / FT), (unsigned)((g.H + FT - 1) / FT), (unsigned)L.m);
    const double* wplane = md.multi() ? w.cw.get() : (md.weighted ? w.wt.get() : nullptr);
    const double* grms = md.multi() ? w.fgrms : w.grms;
    const int absolute = md.absolute ? 1 : 0;
    if (md.matched)
      hipLaunchKernelGGL((filter_kernel<true, true>), grid, dim3(DT), 0, s, w.v, wplane, g.H, g.W, w.kdev, taps.kh, taps.kw, grms,
                         p.thresh, absolute, w.D, w.par);
    else if (wplane)
      hipLaunchKernelGGL((filter_kernel<true, false>), grid, dim3(DT), 0, s, w.v, wplane, g.H, g.W, w.kdev, taps.kh, taps.kw, grms,
                         p.thresh, absolute, w.D, w.par);
    else
      hipLaunchKernelGGL((filter_kernel<false, false>), grid, dim3(DT), 0, s, w.v, nullptr, g.H, g.W, w.kdev, taps.kh, taps.kw,
                         grms, p.thresh, 0, w.D, w.par);
    DV_HIP(hipGetLastError());
    return OK;
  }

  // 6. the components: union-find, labels with areas and boxes, the table of those of >= minarea pixels, the labels map
  int components(const DetectLaunch& L) {
    const long px = L.px, HW = g.HW;
    const dim3 gpix(nblk(px)), blk(DT);
    DV_HIP(hipMemsetAsync(w.area, 0, (size_t)px * sizeof(int), s));
    DV_HIP(hipMemsetAsync(w.cmin, 0x7f, (size_t)px * sizeof(int), s));
    DV_HIP(hipMemsetAsync(w.cmax, 0xff, (size_t)px * sizeof(int), s));
    DV_HIP(hipMemsetAsync(w.rmax, 0xff, (size_t)px * sizeof(int), s));
    hipLaunchKernelGGL(cc_merge_kernel, gpix, blk, 0, s, w.par, px, g.W, HW);
    DV_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_flatten_kernel, gpix, blk, 0, s, w.par, px, g.W, HW, w.lab, w.area, w.cmin, w.cmax, w.rmax);
    DV_HIP(hipGetLastError());
    hipLaunchKernelGGL(cc_compact_kernel, dim3((unsigned)L.m), blk, 0, s, w.lab, w.area, w.cmin, w.cmax, w.rmax, HW, p.minarea,
                       g.ccap, w.table, w.ncomp);
    DV_HIP(hipGetLastError());
    if (md.labels) {
      hipLaunchKernelGGL(cc_labels_kernel, gpix, blk, 0, s, w.lab, w.area, px, HW, p.minarea, w.labout);
      DV_HIP(hipGetLastError());
    }
    return OK;
  }

  int to_host(void* dst, const void* src, size_t bytes) {
    DV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    return OK;
  }
  // 7a. the launch's per-field outputs and maps to the caller's arrays at field f0 (7za: at f0 * k, the back / rms maps
  // [..][k]), the component counts to h_ncomp; returns with the stream idle
  int copy_out(const DetectLaunch& L) {
    const DetectWeights* wq = rq.weights;
    const DetectBands* mb = rq.bands;
    const size_t f0 = (size_t)L.f0, at = f0 * g.HW, px = (size_t)L.px, m = (size_t)L.m, mk = (size_t)L.mk, kk = (size_t)md.kk();
    DV_TRY(to_host(rq.cat.globalrms_h + f0, mb ? w.fgrms : w.grms, m * 8));
    if (mb) {
      if (mb->band_grms_h) DV_TRY(to_host(mb->band_grms_h + f0 * kk, w.grms, mk * 8));
      if (mb->bad_meshes_h && md.planes) DV_TRY(to_host(mb->bad_meshes_h + f0 * kk, w.nbad, mk * 4));
      if (mb->bad_meshes_h && !md.planes) std::fill(mb->bad_meshes_h + f0 * kk, mb->bad_meshes_h + f0 * kk + mk, 0);
      if (mb->V_h) DV_TRY(to_host(mb->V_h + at, w.v, px * 8));
      if (mb->Wt_h) DV_TRY(to_host(mb->Wt_h + at, w.cw, px * 8));
    }
    DV_TRY(to_host(h_ncomp.data(), w.ncomp, m * 4));
    if (wq && wq->bad_meshes_h) DV_TRY(to_host(wq->bad_meshes_h + f0, w.nbad, m * 4));
    if (rq.back_h) DV_TRY(to_host(rq.back_h + at * kk, w.back, px * kk * 8));
    if (rq.rms_h) DV_TRY(to_host(rq.rms_h + at * kk, w.rms, px * kk * 8));
    if (rq.D_h) DV_TRY(to_host(rq.D_h + at, w.D, px * 8));
    if (rq.labels_h) DV_TRY(to_host(rq.labels_h + at, w.labout, px * 4));
    DV_HIP(hipStreamSynchronize(s));
    return OK;
  }

  // 7b. phase two: every field's component table in one synchronisation, then every component's scratch and catalog slots
  int job_table(const DetectLaunch& L, DetectJobs& J) {
    std::vector<long> tab_off((size_t)L.m + 1, 0);
    for (int f = 0; f < L.m; ++f) tab_off[f + 1] = tab_off[f] + h_ncomp[f];
    std::vector<int> h_tab((size_t)std::max(tab_off[L.m], 1L) * 5);
    for (int f = 0; f < L.m; ++f)
      if (h_ncomp[f] > 0) DV_TRY(to_host(h_tab.data() + tab_off[f] * 5, w.table + (long)f * g.ccap * 5, (size_t)h_ncomp[f] * 5 * 4));
    DV_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < L.m; ++f) {
      for (int c = 0; c < h_ncomp[f]; ++c) {
        const int* row = &h_tab[(size_t)(tab_off[f] + c) * 5];
        DbJob j{};
        j.fbase = (long)f * g.HW;
        j.root = row[0]; j.n = row[1]; j.c0 = row[2]; j.c1 = row[3]; j.r1 = row[4];
        j.cap = std::max(1, j.n / p.minarea);
        j.T = md.absolute ? p.thresh : p.thresh * rq.cat.globalrms_h[L.f0 + f];
        j.dws = J.dws; j.iws = J.iws; j.slot = J.slots;
        J.dws += (long)j.n + (long)j.cap * (2 + OBJ_D);
        J.iws += 6L * j.n + 3L * j.cap;
        J.slots += j.cap;
        J.jobs.push_back(j);
        J.jfield.push_back(L.f0 + f);
      }
    }
    J.nj = (long)J.jobs.size();
    return OK;
  }

  // 9. the launch's segmap holds ranks within the component: add every job's base, the objects of its field's earlier
  // components (d.jbase must outlive the kernel: returns with the stream idle)
  int segmap_base(const DetectLaunch& L, const DetectJobs& J, const DetectSlots& h, DeblendScratch& d) {
    std::vector<int> jb((size_t)J.nj);
    int run = 0;
    for (long j = 0; j < J.nj; ++j) {
      if (j > 0 && J.jfield[j] != J.jfield[j - 1]) run = 0;
      jb[j] = run;
      run += h.nobj[j];
    }
    DV_HIP(hipMemcpyAsync(d.jbase, jb.data(), (size_t)J.nj * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(seg_base_kernel, dim3(nblk(L.px)), dim3(DT), 0, s, w.seg, w.lidx, d.jbase, L.px);
    DV_HIP(hipGetLastError());
    DV_HIP(hipStreamSynchronize(s));                      // (jb and the scratch leave scope)
    return OK;
  }
  // 9b. (7zc) the cleaning pass: the launch's raw objects in catalogue order go up as tables, the four kernels run on D and
  // the numbered segmap, and every object's root, new row and mthresh come back; returns with the stream idle
  int clean(const DetectLaunch& L, const DetectJobs& J, const DetectSlots& h, DetectCleaned& c) {
    std::vector<int> up;                                  // rfield | rbox | rnum | rnpix | fptr
    std::vector<double> upd;                              // rd | fT
    std::vector<int> rfield, rbox, rnum, rnpix;
    c.fptr.assign((size_t)L.m + 1, 0);
    std::vector<double> rd, fT((size_t)L.m);
    long ji = 0;
    for (int f = 0; f < L.m; ++f) {
      fT[f] = md.absolute ? p.thresh : p.thresh * rq.cat.globalrms_h[L.f0 + f];
      int k = 0;
      for (; ji < J.nj && J.jfield[ji] == L.f0 + f; ++ji) {
        for (int o = 0; o < h.nobj[ji]; ++o) {
          const long sl = J.jobs[ji].slot + o;
          rfield.push_back(f);
          rbox.insert(rbox.end(), h.oi.begin() + sl * OBJ_I, h.oi.begin() + sl * OBJ_I + 4);
          rnum.push_back(++k);
          rnpix.push_back(h.npix[sl]);
          rd.insert(rd.end(), h.od.begin() + sl * DET_OBJ_D + 1, h.od.begin() + (sl + 1) * DET_OBJ_D);
        }
      }
      c.fptr[f + 1] = (int)rfield.size();
    }
    const size_t n = rfield.size(), nf = (size_t)L.m;
    c.root.resize(n); c.newrow.resize(n); c.mthresh.resize(n);
    if (n == 0) return OK;
    for (const std::vector<int>* v : {&rfield, &rbox, &rnum, &rnpix, &c.fptr}) up.insert(up.end(), v->begin(), v->end());
    upd = rd;
    upd.insert(upd.end(), fT.begin(), fT.end());
    DevBuf<int> ib;
    DevBuf<double> db;
    DV_TRY(ib.alloc(CLEAN_ROW_INTS * n + 2 * nf + 1));
    DV_TRY(db.alloc(CLEAN_ROW_DOUBLES * n + nf));
    DV_HIP(hipMemcpyAsync(ib, up.data(), up.size() * 4, hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(db, upd.data(), upd.size() * 8, hipMemcpyHostToDevice, s));
    int* i0 = ib;
    double* d0 = db;
    CleanTables t{};
    t.D = w.D; t.seg = w.seg; t.W = g.W; t.HW = g.HW; t.n = (int)n; t.nf = (int)nf;
    t.rfield = i0; t.rbox = i0 + n; t.rnum = i0 + 5 * n; t.rnpix = i0 + 6 * n; t.fptr = i0 + 7 * n;
    int* iw = i0 + 7 * n + nf + 1;
    t.absorber = iw; t.root = iw + n; t.rootout = iw + 3 * n; t.newrow = iw + 4 * n; t.nsurv = iw + 5 * n;
    t.rd = d0; t.fT = d0 + 6 * n;
    t.mthresh = d0 + 6 * n + nf; t.der = d0 + 7 * n + nf;
    DV_TRY(detect_clean_launch(t, w.seg, L.px, p.minarea, rq.clean->clean_param, s));
    DV_TRY(to_host(c.root.data(), t.rootout, n * 4));
    DV_TRY(to_host(c.newrow.data(), t.newrow, n * 4));
    DV_TRY(to_host(c.mthresh.data(), t.mthresh, n * 8));
    DV_HIP(hipStreamSynchronize(s));                      // (the tables leave scope)
    return OK;
  }
  // 8. the deblend launch over the launch's jobs and its read-back into h, then (9) the segmap to the caller's array at f0
  int deblend(const DetectLaunch& L, DetectJobs& J, DetectSlots& h, DetectCleaned& cl) {
    const size_t nj = (size_t)J.nj, slots = (size_t)J.slots;
    h.nobj.resize(nj); h.npix.resize(slots);
    for (std::vector<double>* v : {&h.peak, &h.flux, &h.x, &h.y}) v->resize(slots);
    if (md.objects) { h.oi.resize(slots * OBJ_I); h.od.resize(slots * DET_OBJ_D); }
    if (md.segmap) DV_HIP(hipMemsetAsync(w.seg, 0, (size_t)L.px * sizeof(int), s));
    if (nj > 0) {
      DeblendScratch d;
      DV_TRY(d.alloc(J.nj, J.dws, J.iws, J.slots, md.objects));
      if (md.objects) {                                   // the request rides behind the jobs, in the place of one more
        const DbObjects oo{md.multi() ? w.cw.get() : (md.weighted ? w.wt.get() : nullptr), g.H,
                           md.segmap ? w.seg.get() : nullptr, d.oi, d.od};
        J.jobs.push_back(DbJob{});
        std::memcpy(&J.jobs[nj], &oo, sizeof(oo));
      }
      DV_HIP(hipMemcpyAsync(d.djobs, J.jobs.data(), J.jobs.size() * sizeof(DbJob), hipMemcpyHostToDevice, s));
      if (md.objects) {
        DV_TRY(deblend_objects_launch(J.nj, s, d.djobs, g.W, w.D, w.v, w.lab, w.lidx, d.dscr, d.iscr, p.nthresh, p.minarea, p.cont,
                                      d.o_npix, d.o_pp, d.o_peak, d.o_flux, d.o_x, d.o_y, d.nobj));
      } else {
        hipLaunchKernelGGL(deblend_kernel<false>, dim3((unsigned)nj), dim3(DT), 0, s, d.djobs, g.W, w.D, w.v, w.lab, w.lidx, d.dscr,
                           d.iscr, p.nthresh, p.minarea, p.cont, d.o_npix, d.o_pp, d.o_peak, d.o_flux, d.o_x, d.o_y, d.nobj);
      }
      DV_HIP(hipGetLastError());
      if (md.objects) {
        DV_TRY(to_host(h.oi.data(), d.oi, h.oi.size() * 4));
        DV_TRY(to_host(h.od.data(), d.od, h.od.size() * 8));
      }
      DV_TRY(to_host(h.nobj.data(), d.nobj, nj * 4));
      DV_TRY(to_host(h.npix.data(), d.o_npix, slots * 4));
      DV_TRY(to_host(h.peak.data(), d.o_peak, slots * 8));
      DV_TRY(to_host(h.flux.data(), d.o_flux, slots * 8));
      DV_TRY(to_host(h.x.data(), d.o_x, slots * 8));
      DV_TRY(to_host(h.y.data(), d.o_y, slots * 8));
      DV_HIP(hipStreamSynchronize(s));
      if (md.segmap) DV_TRY(segmap_base(L, J, h, d));
      if (md.clean) DV_TRY(clean(L, J, h, cl));
    }
    if (rq.objects && rq.objects->segmap_h) {
      DV_TRY(to_host(rq.objects->segmap_h + (size_t)L.f0 * g.HW, w.seg, (size_t)L.px * 4));
      DV_HIP(hipStreamSynchronize(s));
    }
    return OK;
  }

  // 10. the launch's objects behind the catalogue, field by field, and the fields' offsets
  void append_catalogue(const DetectLaunch& L, const DetectJobs& J, const DetectSlots& h, const DetectCleaned& cl) {
    long ji = 0;
    for (int f = 0; f < L.m; ++f) {
      const size_t row0 = cat.field.size();
      for (; ji < J.nj && J.jfield[ji] == L.f0 + f; ++ji) {
        for (int o = 0; o < h.nobj[ji]; ++o) {
          const long sl = J.jobs[ji].slot + o;
          cat.field.push_back(L.f0 + f);
          cat.parent.push_back(J.jobs[ji].root);
          cat.npix.push_back(h.npix[sl]);
          cat.peak.push_back(h.peak[sl]);
          cat.flux.push_back(h.flux[sl]);
          cat.x.push_back(h.x[sl]);
          cat.y.push_back(h.y[sl]);
          if (md.objects) {
            cat.oi.insert(cat.oi.end(), h.oi.begin() + sl * OBJ_I, h.oi.begin() + sl * OBJ_I + DET_OBJ_I);
            cat.od.insert(cat.od.end(), h.od.begin() + sl * DET_OBJ_D, h.od.begin() + (sl + 1) * DET_OBJ_D);
          }
        }
      }
      if (md.clean) {
        if (rq.clean->n_raw_h) rq.clean->n_raw_h[L.f0 + f] = (int64_t)(cat.field.size() - row0);
        if (!cl.fptr.empty()) merge_cleaned(row0, cl, cl.fptr[f]);
      }
      rq.cat.offsets_h[L.f0 + f + 1] = (int64_t)cat.field.size();
    }
  }

  // (7zc) the raw rows of one field, the catalogue's from row0 on (raw object r0 of the launch first), become its cleaned rows:
  // the survivors in order, every victim merged into its root in ascending raw row (sep's mergeobject)
  void merge_cleaned(size_t row0, const DetectCleaned& cl, int r0) {
    const size_t n = cat.field.size() - row0;
    cat.nmerged.resize(row0 + n, 1);
    cat.mthresh.resize(row0 + n, 0.0);
    bool any = false;
    for (size_t r = 0; r < n; ++r) {
      cat.mthresh[row0 + r] = cl.mthresh[r0 + r];
      any = any || cl.root[r0 + r] != r0 + (int)r;
    }
    if (!any) return;                                     // nothing absorbed: the rows stay as they are, bit for bit
    HostCatalog raw;
    const auto take = [&](auto& dst, const auto& src, size_t width) {
      dst.assign(src.begin() + row0 * width, src.end());
    };
    take(raw.field, cat.field, 1); take(raw.parent, cat.parent, 1); take(raw.npix, cat.npix, 1); take(raw.peak, cat.peak, 1);
    take(raw.flux, cat.flux, 1); take(raw.x, cat.x, 1); take(raw.y, cat.y, 1); take(raw.oi, cat.oi, DET_OBJ_I);
    take(raw.od, cat.od, DET_OBJ_D); take(raw.mthresh, cat.mthresh, 1);
    // surv[k]: the raw row of survivor k; the victims join in ascending raw row
    std::vector<size_t> surv;
    for (size_t r = 0; r < n; ++r)
      if (cl.root[r0 + r] == r0 + (int)r) surv.push_back(r);
    cat.truncate(row0);
    for (size_t r : surv) {
      cat.field.push_back(raw.field[r]); cat.parent.push_back(raw.parent[r]); cat.npix.push_back(raw.npix[r]);
      cat.peak.push_back(raw.peak[r]); cat.flux.push_back(raw.flux[r]); cat.x.push_back(raw.x[r]); cat.y.push_back(raw.y[r]);
      cat.oi.insert(cat.oi.end(), raw.oi.begin() + r * DET_OBJ_I, raw.oi.begin() + (r + 1) * DET_OBJ_I);
      cat.od.insert(cat.od.end(), raw.od.begin() + r * DET_OBJ_D, raw.od.begin() + (r + 1) * DET_OBJ_D);
      cat.nmerged.push_back(1); cat.mthresh.push_back(raw.mthresh[r]);
    }
    std::vector<size_t> pk = surv, vk = surv;
    for (size_t r = 0; r < n; ++r) {
      if (cl.root[r0 + r] == r0 + (int)r) continue;
      const size_t k = row0 + (size_t)cl.newrow[r0 + r];
      int32_t* si = &cat.oi[k * DET_OBJ_I];
      double* sd = &cat.od[k * DET_OBJ_D];
      const int32_t* vi = &raw.oi[r * DET_OBJ_I];
      const double* vd = &raw.od[r * DET_OBJ_D];
      cat.npix[k] += raw.npix[r];
      cat.flux[k] += raw.flux[r];
      sd[1] += vd[1];                                      // dflux
      // the largest value, a tie to the earlier raw row: pk / vk hold the raw row the merged row's peak / vpeak come from
      if (raw.peak[r] > cat.peak[k] || (raw.peak[r] == cat.peak[k] && r < pk[k - row0])) {
        cat.peak[k] = raw.peak[r]; si[4] = vi[4]; si[5] = vi[5];
        pk[k - row0] = r;
      }
      if (vd[0] > sd[0] || (vd[0] == sd[0] && r < vk[k - row0])) {
        sd[0] = vd[0]; si[6] = vi[6]; si[7] = vi[7];
        vk[k - row0] = r;
      }
      si[0] = std::min(si[0], vi[0]); si[1] = std::max(si[1], vi[1]);
      si[2] = std::min(si[2], vi[2]); si[3] = std::max(si[3], vi[3]);
      si[8] |= vi[8] | DV_DETECT_FLAG_MERGED;
      ++cat.nmerged[k];
    }
  }

  // the count always, the rows when they fit into the caller's cap
  void write_catalogue() {
    const DetectCatalog& out = rq.cat;
    const size_t n = cat.field.size();
    *out.n_out = (int64_t)n;
    if ((int64_t)n > out.cap || n == 0) return;
    std::copy(cat.field.begin(), cat.field.end(), out.field_h);
    std::copy(cat.parent.begin(), cat.parent.end(), out.parent_h);
    std::copy(cat.npix.begin(), cat.npix.end(), out.npix_h);
    std::copy(cat.peak.begin(), cat.peak.end(), out.peak_h);
    std::copy(cat.flux.begin(), cat.flux.end(), out.flux_h);
    std::copy(cat.x.begin(), cat.x.end(), out.x_h);
    std::copy(cat.y.begin(), cat.y.end(), out.y_h);
    if (md.clean) {
      if (rq.clean->nmerged_h) std::copy(cat.nmerged.begin(), cat.nmerged.end(), rq.clean->nmerged_h);
      if (rq.clean->mthresh_h) std::copy(cat.mthresh.begin(), cat.mthresh.end(), rq.clean->mthresh_h);
    }
    if (!rq.objects) return;
    for (size_t i = 0; i < n; ++i) {
      for (int e = 0; e < DET_OBJ_I; ++e)
        if (rq.objects->icol[e]) rq.objects->icol[e][i] = cat.oi[i * DET_OBJ_I + e];
      for (int e = 0; e < DET_OBJ_D; ++e)
        if (rq.objects->dcol[e]) rq.objects->dcol[e][i] = cat.od[i * DET_OBJ_D + e];
    }
  }
};
}  // namespace

int detect_bands_check(const char* who, const int32_t* bands, int k, const double* c, int nb, int noise, int filter) {
  if (nb < 1 || k < 1 || k > nb || !bands) {
    set_error("%s: %d band(s) selected, 1 .. %d of the fields' must be given", who, k, nb);
    return E_INVALID;
  }
  for (int j = 0; j < k; ++j) {
    if (bands[j] < 0 || bands[j] >= nb) {
      set_error("%s: band %d is outside the fields' %d band(s)", who, bands[j], nb);
      return E_INVALID;
    }
    for (int i = 0; i < j; ++i)
      if (bands[i] == bands[j]) {
        set_error("%s: band %d is given twice", who, bands[j]);
        return E_INVALID;
      }
    if (c && !(c[j] > 0.0 && std::isfinite(c[j]))) {
      set_error("%s: band weight %d must be finite and > 0 (got %g)", who, j, c[j]);
      return E_INVALID;
    }
  }
  if ((noise != 0 && noise != 1) || (filter != 0 && filter != 1)) {
    set_error("%s: noise must be 0 (absolute) or 1 (relative) and filter 0 (conv) or 1 (matched), got %d, %d", who, noise, filter);
    return E_INVALID;
  }
  return OK;
}

int scene_detect(const DetectRequest& rq, hipStream_t s) {
  DV_TRY(detect_check(rq));
  const dv_detect_params& p = *rq.par;
  DetectTaps taps;
  DV_TRY(detect_taps(p, taps));
  const int M = rq.M;
  const long HW = (long)rq.H * rq.W;
  DetectRun run{rq, p, detect_mode(rq), DetectGeom{rq.H, rq.W, (rq.H + p.back_size - 1) / p.back_size,
                                                   (rq.W + p.back_size - 1) / p.back_size, HW, HW / p.minarea + 1}, taps, s};
  const long cap_ws = p.workspace_bytes > 0 ? (long)p.workspace_bytes : (4L << 30);
  const long per_field = field_bytes(run.g, run.md);
  if (M > 0 && per_field > cap_ws) {
    set_error("scene_detect: one %d x %d field needs up to %ld bytes of device workspace, above the cap of %ld bytes per "
              "launch", rq.H, rq.W, per_field, cap_ws);
    return E_INVALID;
  }
  const int chunk = M > 0 ? (int)std::min<long>({(long)M, (long)CHUNK_MAX, std::max<long>(1, cap_ws / per_field)}) : 0;
  rq.cat.offsets_h[0] = 0;
  DV_TRY(run.prepare(chunk));
  for (int f0 = 0; f0 < M; f0 += chunk) {
    const int m = std::min(chunk, M - f0);
    const DetectLaunch L{f0, m, (long)m * HW, m * run.md.kk()};
    DV_TRY(run.load_planes(L));
    DV_TRY(run.background(L));
    DV_TRY(run.filter(L));
    DV_TRY(run.components(L));
    DV_TRY(run.copy_out(L));
    DetectJobs jobs;
    DetectSlots slots;
    DetectCleaned cleaned;
    DV_TRY(run.job_table(L, jobs));
    DV_TRY(run.deblend(L, jobs, slots, cleaned));
    run.append_catalogue(L, jobs, slots, cleaned);
  }
  run.write_catalogue();
  return OK;
}

}  // namespace dv
