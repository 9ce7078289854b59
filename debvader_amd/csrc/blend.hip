// Blendedness sums of deblended galaxies: how much of the light under a galaxy's own weight belongs to its
// neighbours.  The reference ships an empty debvader.measure package; the quantity is defined here, after the blendedness
// of Bosch et al. 2018 (4.9.11) without its clipping.
//
// Per galaxy, float64 throughout: P its mean stamp [cs][cs][nb] (float32 widened), {r0, c0, Mrr, Mrc, Mcc} and status its
// catalogue row (measure.hip), (pr, pc) its placement, T the composited mean field of its field [F][F][nb], D the observed
// field.  Eligible: status 0 or 2, five finite shape values, det = Mrr Mcc - Mrc^2 finite and above 1e-6 (measure_stamp's
// threshold).  Over the stamp pixels that lie inside the field (the composite drops the others), with
//   g = exp(qa dr^2 + qb dr dc + qc dc^2), dr = r - r0, dc = c - c0, qa = -Mcc / (2 det), qb = Mrc / det, qc = -Mrr / (2 det)
//   W = sum g    A = sum g P[r, c, band]    Bm = sum g T[pr + r, pc + c, band]    Bd = sum g D[pr + r, pc + c, band]
// and npix = the number of pixels summed.  An ineligible row gets four NaN and npix = -1.
//
// Two kernels, one workgroup of 256 threads per galaxy each, one pass, reduction scratch only (64 B of LDS):
//   blend_child_kernel   W, A, npix - needs the stamp, which lies in HBM only while its chunk does;
//   blend_parent_kernel  Bm, Bd     - needs the field's finished composite; reads the resident catalogue rows, the
//                                     placements, the mean field and the source field.  One band out of [F][F][nb] doubles:
//                                     a stride of nb * 8 bytes along a row, every 64-byte line fetched for one double of it.
//                                     Once per galaxy, not per iteration.
// Both walk the stamp with the same assignment of pixels to threads (pixel e = r * cs + c belongs to thread e mod 256, in
// ascending e), compute g by the same inlined function, and reduce as measure.hip does: butterfly within the wave, then
// through LDS in wave order.  Floating-point contraction is off in this file: every product and every sum is rounded on its
// own, so g and the order of additions are the same in both kernels whatever the compiler does with either.  Hence a
// galaxy's row has the same bits wherever it sits in a batch, and for a galaxy alone in its field - T holds exactly its
// widened stamp values - A and Bm have the same bits.  No atomics; thread 0 writes with ordinary stores.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace dv {

namespace {
constexpr int BL_THREADS = 256;

struct BlWeight { double r0, c0, qa, qb, qc; };

// the weight of a catalogue row; false: the row is ineligible (the same answer in every thread of the workgroup)
__device__ __forceinline__ bool bl_weight(const double* __restrict__ sh, int st, BlWeight& w) {
  if (st != 0 && st != 2) return false;
  const double r0 = sh[0], c0 = sh[1], Mrr = sh[2], Mrc = sh[3], Mcc = sh[4];
  if (!(ms_finite(r0) && ms_finite(c0) && ms_finite(Mrr) && ms_finite(Mrc) && ms_finite(Mcc))) return false;
  const double det = Mrr * Mcc - Mrc * Mrc;
  if (!(ms_finite(det) && det > 1e-6)) return false;
  w.r0 = r0;
  w.c0 = c0;
  w.qa = -0.5 * Mcc / det;
  w.qb = Mrc / det;
  w.qc = -0.5 * Mrr / det;
  return true;
}

__device__ __forceinline__ double bl_gauss(const BlWeight& w, int r, int c) {
  const double dr = (double)r - w.r0, dc = (double)c - w.c0;
  return exp(w.qa * dr * dr + w.qb * dr * dc + w.qc * dc * dc);
}

// stamps [n][cs][cs][nb] float32; shape [n][5], status [n], places [n][2], blend [n][4], npix [n]: the rows of the n stamps
__global__ __launch_bounds__(BL_THREADS) void blend_child_kernel(const float* __restrict__ stamps,
                                                                 const double* __restrict__ shape,
                                                                 const int* __restrict__ status,
                                                                 const int* __restrict__ places, int cs, int nb, int band,
                                                                 int F, double* __restrict__ blend, int* __restrict__ npix) {
  __shared__ double s_red[4 * 2];
  const long gi = blockIdx.x;
  BlWeight w;
  if (!bl_weight(shape + gi * 5, status[gi], w)) {     // (uniform: every thread read the same row)
    if (threadIdx.x == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      blend[gi * 4 + 0] = blend[gi * 4 + 1] = blend[gi * 4 + 2] = blend[gi * 4 + 3] = nan;
      npix[gi] = -1;
    }
    return;
  }
  const int pr = places[2 * gi], pc = places[2 * gi + 1];
  const float* P = stamps + gi * cs * cs * nb + band;
  double a[2] = {0.0, 0.0};
  for (int e = threadIdx.x; e < cs * cs; e += BL_THREADS) {
    const int r = e / cs, c = e - r * cs;
    if ((unsigned)(pr + r) >= (unsigned)F || (unsigned)(pc + c) >= (unsigned)F) continue;
    const double g = bl_gauss(w, r, c);
    a[0] += g;
    a[1] += g * (double)P[(long)e * nb];
  }
  ms_block_sum<2>(a, s_red);
  if (threadIdx.x == 0) {
    // rows / columns of the stamp inside the field: [max(0, -p), min(cs, F - p))
    const int nr = min(cs, F - pr) - max(0, -pr), nc = min(cs, F - pc) - max(0, -pc);
    blend[gi * 4 + 0] = a[0];
    blend[gi * 4 + 1] = a[1];
    npix[gi] = nr > 0 && nc > 0 ? nr * nc : 0;
  }
}

// the rows of n galaxies whose fields are complete; sfield [n] their fields, model / data the stacks from field f0 on
__global__ __launch_bounds__(BL_THREADS) void blend_parent_kernel(const double* __restrict__ shape,
                                                                  const int* __restrict__ status,
                                                                  const int* __restrict__ places,
                                                                  const int* __restrict__ sfield, int f0, int cs, int nb,
                                                                  int band, int F, const double* __restrict__ model,
                                                                  const double* __restrict__ data,
                                                                  double* __restrict__ blend) {
  __shared__ double s_red[4 * 2];
  const long gi = blockIdx.x;
  BlWeight w;
  if (!bl_weight(shape + gi * 5, status[gi], w)) return;   // (the child pass wrote the row's NaN)
  const int pr = places[2 * gi], pc = places[2 * gi + 1];
  const long fo = (long)(sfield[gi] - f0) * F * F * nb + band;
  const double* T = model + fo;
  const double* D = data ? data + fo : nullptr;
  double a[2] = {0.0, 0.0};
  for (int e = threadIdx.x; e < cs * cs; e += BL_THREADS) {
    const int r = e / cs, c = e - r * cs;
    if ((unsigned)(pr + r) >= (unsigned)F || (unsigned)(pc + c) >= (unsigned)F) continue;
    const double g = bl_gauss(w, r, c);
    const long fe = ((long)(pr + r) * F + (pc + c)) * nb;
    a[0] += g * T[fe];
    if (D) a[1] += g * D[fe];
  }
  ms_block_sum<2>(a, s_red);
  if (threadIdx.x == 0) {
    blend[gi * 4 + 2] = a[0];
    blend[gi * 4 + 3] = D ? a[1] : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// mean_f += the chunk's mean stamps at their placements, per field element in object order: the additions of
// scene_composite_chunk_kernel's mean sum, one thread per field pixel, every field scanning its own objects of the chunk
// (fptr[m] .. fptr[m + 1] cut to [obase, obase + n)).  A pixel no object covers is not written.
__global__ __launch_bounds__(256) void blend_composite_mean_kernel(double* __restrict__ mean_f, int F, int nb,
                                                                   const float* __restrict__ loc,
                                                                   const int* __restrict__ places, int n, int cs,
                                                                   const int* __restrict__ fptr, int f0, int fy0,
                                                                   long obase) {
  const int m = fy0 + (int)blockIdx.y;
  const long lo = (long)fptr[m] - obase, hi = (long)fptr[m + 1] - obase;
  const int olo = (int)(lo > 0 ? lo : 0);
  n = (int)(hi < n ? hi : n);
  if (olo >= n) return;
  const long px = (long)blockIdx.x * 256 + threadIdx.x;
  if (px >= (long)F * F) return;
  const int r = (int)(px / F), c = (int)(px - (long)r * F);
  double* dst = mean_f + ((long)(m - f0) * F * F + px) * nb;
  for (int o = olo; o < n; ++o) {
    const int rr = r - places[2 * o], cc = c - places[2 * o + 1];
    if ((unsigned)rr < (unsigned)cs && (unsigned)cc < (unsigned)cs) {
      const float* src = loc + (((long)o * cs + rr) * cs + cc) * nb;
      for (int b = 0; b < nb; ++b) dst[b] += (double)src[b];
    }
  }
}

// ---- the end-of-loop sums of a resident field set (dv_field_set_blend) ------------------------------------
// Row gi of the set's resident rows (shape, status, places, sfield: every stamp of every measured pass, in call order)
// against the set's stacks as they are now: sums [n][4] = {Bm, Bd, R1, R2} = sum g mean, sum g base, sum g final,
// sum g (final final) over the stamp pixels inside the field - the pixels, the weight and the eligibility of the two
// kernels above.  One walk of the footprint reads the three stacks at the same field element; the square is a product of
// its own, rounded before it meets g.  The first two sums are blend_parent_kernel's operations in its order (the block sum
// treats every k on its own), so they have its bits for the same row and stacks.  base null (a cumulative set keeps none):
// Bd is NaN.  An ineligible row gets four NaN.
__global__ __launch_bounds__(BL_THREADS) void blend_set_kernel(const double* __restrict__ shape,
                                                               const int* __restrict__ status,
                                                               const int* __restrict__ places,
                                                               const int* __restrict__ sfield, int cs, int nb, int band,
                                                               int F, const double* __restrict__ mean,
                                                               const double* __restrict__ base,
                                                               const double* __restrict__ fin, double* __restrict__ sums) {
  __shared__ double s_red[4 * 4];
  const long gi = blockIdx.x;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  BlWeight w;
  if (!bl_weight(shape + gi * 5, status[gi], w)) {     // (uniform: every thread read the same row)
    if (threadIdx.x == 0) sums[gi * 4 + 0] = sums[gi * 4 + 1] = sums[gi * 4 + 2] = sums[gi * 4 + 3] = nan;
    return;
  }
  const int pr = places[2 * gi], pc = places[2 * gi + 1];
  const long fo = (long)sfield[gi] * F * F * nb + band;
  const double* T = mean + fo;
  const double* D = base ? base + fo : nullptr;
  const double* R = fin + fo;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = threadIdx.x; e < cs * cs; e += BL_THREADS) {
    const int r = e / cs, c = e - r * cs;
    if ((unsigned)(pr + r) >= (unsigned)F || (unsigned)(pc + c) >= (unsigned)F) continue;
    const double g = bl_gauss(w, r, c);
    const long fe = ((long)(pr + r) * F + (pc + c)) * nb;
    a[0] += g * T[fe];
    if (D) a[1] += g * D[fe];
    const double x = R[fe];
    const double xx = x * x;
    a[2] += g * x;
    a[3] += g * xx;
  }
  ms_block_sum<4>(a, s_red);
  if (threadIdx.x == 0) {
    sums[gi * 4 + 0] = a[0];
    sums[gi * 4 + 1] = D ? a[1] : nan;
    sums[gi * 4 + 2] = a[2];
    sums[gi * 4 + 3] = a[3];
  }
}
}  // namespace

// the refusals of the stamp-level call, before any GPU work: the kernels hold nothing per pixel, so the sizes are bounded
// by their 32-bit pixel indices alone
int blend_check(const char* who, int cs, int nb, int band) {
  if (cs < 1 || cs > 4096 || nb < 1 || nb > 4096) {
    set_error("%s: stamps of %d pixels and %d bands; 1 .. 4096 pixels and 1 .. 4096 bands are taken", who, cs, nb);
    return E_INVALID;
  }
  if (band < 0 || band >= nb) {
    set_error("%s: band %d asked for, the stamps have bands 0 .. %d", who, band, nb - 1);
    return E_INVALID;
  }
  return OK;
}

int launch_blend_child(const float* stamps_dev, const double* shape_dev, const int* status_dev, const int* places_dev, int n,
                       int cs, int nb, int band, int F, double* blend_dev, int* npix_dev, hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(blend_child_kernel, dim3((unsigned)n), dim3(BL_THREADS), 0, s, stamps_dev, shape_dev, status_dev,
                     places_dev, cs, nb, band, F, blend_dev, npix_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_blend_parent(const double* shape_dev, const int* status_dev, const int* places_dev, const int* sfield_dev, int f0,
                        int n, int cs, int nb, int band, int F, const double* model_dev, const double* data_dev,
                        double* blend_dev, hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(blend_parent_kernel, dim3((unsigned)n), dim3(BL_THREADS), 0, s, shape_dev, status_dev, places_dev,
                     sfield_dev, f0, cs, nb, band, F, model_dev, data_dev, blend_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_blend_composite_mean(double* mean_f, int F, int nb, const float* loc, const int* places_dev, int n, int cs,
                                const int* fptr_dev, int f0, int fy0, int nfields, long obase, hipStream_t s) {
  if (n <= 0) return OK;
  if (nfields < 1 || nfields > 65535) {
    set_error("blend composite: a chunk spans %d fields, at most 65535", nfields);
    return E_INVALID;
  }
  const dim3 grid((unsigned)(((long)F * F + 255) / 256), (unsigned)nfields);
  hipLaunchKernelGGL(blend_composite_mean_kernel, grid, dim3(256), 0, s, mean_f, F, nb, loc, places_dev, n, cs, fptr_dev, f0,
                     fy0, obase);
  DV_HIP(hipGetLastError());
  return OK;
}

// the n resident rows of a field set against its stacks [M][F][F][nb] (sfield counts from field 0); base_dev null: Bd = NaN
int launch_blend_set(const double* shape_dev, const int* status_dev, const int* places_dev, const int* sfield_dev, int n, int cs,
                     int nb, int band, int F, const double* mean_dev, const double* base_dev, const double* final_dev,
                     double* sums_dev, hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(blend_set_kernel, dim3((unsigned)n), dim3(BL_THREADS), 0, s, shape_dev, status_dev, places_dev,
                     sfield_dev, cs, nb, band, F, mean_dev, base_dev, final_dev, sums_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

void blend_columns(Rows& r, BlendRows& dev, const BlendRows& host) {
  r.add(dev.blend, host.blend, 4);
  r.add(dev.npix, host.npix, 1);
}

// host arrays in, host rows out: a chunk of stamps at a time, the model (and data) fields they lie in uploaded beside them
int scene_blend(const float* stamps_h, const double* shape_h, const int32_t* status_h, const int32_t* places_h,
                const int64_t* field_ptr, int64_t N, int cs, int nb, int band, const double* model_h, const double* data_h,
                int M, int F, const BlendRows& out_h, hipStream_t s) {
  const char* who = "dv_scene_blend";
  if (N < 0 || M < 0 || !field_ptr ||
      (N > 0 && (!stamps_h || !shape_h || !status_h || !places_h || !model_h || !out_h.blend || !out_h.npix))) {
    set_error("%s: stamps, shape, status, places, field_ptr, model_fields, blend and npix must all be given", who);
    return E_INVALID;
  }
  std::vector<int32_t> sfield;
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, &sfield, nullptr));
  float* stamps = nullptr;
  double* shape = nullptr;
  int *status = nullptr, *places = nullptr, *sf = nullptr;
  BlendRows d{};
  Rows in, out;
  in.add(stamps, stamps_h, (size_t)cs * cs * nb);
  in.add(shape, shape_h, 5);
  in.add(status, status_h, 1);
  in.add(places, places_h, 2);
  in.add(sf, sfield.data(), 1);
  blend_columns(out, d, out_h);
  FieldStacks f{model_h, data_h, (size_t)F * F * nb, M};
  return walk_field_rows(N, sfield.data(), f, in, out, s, [&](int64_t, int n, int fa) {
    DV_TRY(launch_blend_child(stamps, shape, status, places, n, cs, nb, band, F, d.blend, d.npix, s));
    return launch_blend_parent(shape, status, places, sf, fa, n, cs, nb, band, F, f.model_d, f.data_d, d.blend, s);
  });
}

}  // namespace dv
