// Simultaneous flux fit of the deblended models to the observed field: the shapes of the galaxies of a field
// are held fixed at their mean stamps and all their amplitudes are fitted to the observed pixels at once, per band - the last
// step of the SDSS deblender, the Tractor's and scarlet's flux re-fit.  Linear least squares; the reference ships an empty
// debvader.measure package, so the quantity is defined here.
//
// Float64 throughout, floating-point contraction off: every product and every sum is rounded on its own.  Per field m with
// galaxies i = 0 .. n - 1 in object order: P_i the mean stamp [cs][cs][nb] (float32, widened), (pr_i, pc_i) = places[i], D the
// observed field [F][F][nb].  The pixels of i are the stamp pixels whose field pixel lies inside the field (the pixels the
// composite keeps, 7l).  Per band b, independently:
//   1. G_ij = sum P_i P_j over the field pixels both stamps cover (j <= i), exactly 0.0 where the two clipped rectangles do not
//      intersect; h_i = sum P_i D over the pixels of i.  Every sum is one fixed-order workgroup reduction (ms_block_sum).
//   2. A galaxy whose G_ii is not finite or not positive has status 4: fit_scale and fit_var NaN, not part of the system.
//   3. Cholesky factorisation of G over the eligible galaxies in object order, with dropping: at column k the pivot is
//      d_k = G_kk - sum_{j < k, kept} L_kj^2; d_k <= min_pivot G_kk drops galaxy k (status 5).  A dropped column is never
//      applied to the others: the variable leaves the system.  Of two models that cannot be told apart the one dropped is
//      always the later in object order - the earlier one has been factorised when the later one's pivot vanishes.
//   4. A dropped galaxy keeps the network's amplitude: h'_i = h_i - sum_{k dropped} G_ik, fit_scale = 1, fit_var = NaN.
//   5. G_kept a = h' by the two triangular solves: fit_scale = a; fit_var_i = (G_kept^-1)_ii, the sum of squares of column i
//      of L^-1.  fit_gram = G_ii and fit_proj = h_i are given for every galaxy.  Amplitudes are not clipped.
//
// Two kernels:
//   fitflux_gram_kernel   one 256-thread workgroup per entry of a pair list (i, j <= i) the host builds from the placements:
//                         the pairs of one field whose clipped rectangles intersect, diagonal included.  Threads take the pixels
//                         of the intersection in raster order, stride 256; a pixel reads the nb contiguous floats of both
//                         stamps into statically indexed band slots (8-byte loads where the address allows); one ms_block_sum
//                         per band; thread 0 writes G[b][i][j] of the field's dense scratch [nb][n][n] (lower triangle, zeroed
//                         before the launch).  The diagonal entry also takes h_i against D and writes fit_gram and fit_proj.
//   fitflux_solve_kernel  one workgroup per (field, band): steps 2 - 5 in place on that scratch in global memory.  The strict
//                         upper triangle (transposed) and the diagonal take the working copy that becomes L - column k of L is
//                         contiguous -, the strict lower triangle keeps G for step 4 and then takes L^-1.  The workgroup reads
//                         only what it wrote itself, behind __syncthreads(); nothing is handed between workgroups.  Every
//                         element is updated by one thread per column, in ascending column order, and every other sum runs in
//                         ascending index order in one thread: a field's rows have the same bits wherever the field sits in a
//                         batch and when it is alone.
// The weighted fit takes a weight field W laid out like D, meant as the inverse variance of every pixel.  A pixel
// of band b counts iff 0 < W < inf; every other pixel's terms are exactly +0.0, selected and not multiplied, so nothing under a
// masked pixel reaches a sum.  Step 1 becomes G_ij = sum (W P_i) P_j and h_i = sum (W P_i) D over the counting pixels - the
// product with W first: with W = 1.0 every term has the bits of the unweighted one -, in fitflux_gram_kernel<true>; steps 2 - 5
// run unchanged in fitflux_solve_kernel; then, new:
//   6. per galaxy i and band the chi-square of the refitted scene under the pixels p of i: M(p) = sum_j a_j P_j(p) over the
//      galaxies j of the field, in ascending row order, that cover p and do not have status 4, a_j = fit_scale (1 for a dropped
//      one), summed sequentially in one thread; r = D(p) - M(p); fit_chi2 = sum over the counting p of (W r) r, one fixed-order
//      workgroup reduction, NaN where i has status 4; fit_npix = the number of counting pixels of i, written for every galaxy.
//   fitflux_chi2_kernel   one 256-thread workgroup per galaxy, behind the solve of its sub-range; the neighbours come from a CSR
//                         adjacency the host builds beside the pair list.
// The fit with a sky background fitted jointly adds Q = 1 (a constant) or 3 (a plane) unknowns per field and band
// behind the galaxies, in the basis B_0 = 1, B_1 = (2 r - F + 1) / F, B_2 = (2 c - F + 1) / F of the field pixel (r, c): the
// model is sum a_i P_i + sum s_t B_t over all (counting) pixels of the field, the system [[G, E], [E^T, K]] [a; s] = [h; c] with
// E_it = sum (W P_i) B_t, K_tu = sum (W B_t) B_u, c_t = sum (W B_t) D.  Every kernel is a template on Q, and Q = 0 is the code
// above, instruction for instruction; new:
//   fitflux_border_kernel     one workgroup per galaxy: E_it into row n + t of the field's scratch, whose rows hold n + Q doubles.
//   fitflux_skysum_kernel     K, c and the counting pixels of every field: a streaming reduction over D and W in tiles of 4096
//                             pixels, four bands per workgroup, one row of partial sums per tile;
//   fitflux_skyreduce_kernel  the partial sums in tile order - an order that depends on F alone.
// The sky terms are eliminated last: the factorisation of the galaxy block is the one of the fit without sky, bit for bit.
// The non-negative fit minimises the same quadratic subject to a_i >= 0 for the galaxies, the sky left free:
//   fitflux_nonneg_kernel     in place of fitflux_solve_kernel when the constraint is asked for, on the same scratch: iteration
//                             1 is steps 2 - 5 above, then the active set is exchanged and the kept unknowns that are not
//                             clamped are factorised again until no amplitude and no multiplier is negative.
// The fit by blend groups lifts the limit of FF_MAX_N galaxies from the field to the group: the connected
// components of the graph of adjacent galaxies - the pairs of the list above - are found on the GPU (fitgroups_count / scan /
// fill / label kernels, below) and every group is solved on its own by the GROUPED instantiations of the Gram and solve
// kernels, which reach their rows through group tables; GROUPED = false is the code as it was, instruction for instruction.
// The grouped fit of a resident field set works in place on a stamp store that is not in the order of the call:
// the INDEXED instantiations of the Gram and chi-square kernels read the stamp of row i at stamps + srow[i] cs cs nb; every
// other table, slot and output stays indexed by the row of the call.  INDEXED = false is the code as it was.
// No atomics; ordinary vector stores only.
#include "common.h"
#include "measure_dev.h"
#include "rows.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace dv {

namespace {
constexpr int FF_BANDS = FF_SKY_BANDS;

// the nb floats at p, widened, into the band slots; an 8-byte load for every pair of slots that starts at an aligned address
// (ODD: p itself is 4 bytes past one, slot 0 goes alone).  Slots from nb on are left alone; nothing past p[nb - 1] is read.
template <int ODD>
__device__ __forceinline__ void ff_load_slots(const float* __restrict__ p, int nb, double (&v)[FF_BANDS]) {
  if (ODD) v[0] = (double)p[0];
#pragma unroll
  for (int b = ODD; b < FF_BANDS; b += 2) {
    if (b + 1 < FF_BANDS && b + 1 < nb) {
      const float2 t = *reinterpret_cast<const float2*>(p + b);
      v[b] = (double)t.x;
      v[b + 1 < FF_BANDS ? b + 1 : b] = (double)t.y;
    } else if (b < nb) {
      v[b] = (double)p[b];
    }
  }
}

__device__ __forceinline__ void ff_load(const float* __restrict__ p, int nb, double (&v)[FF_BANDS]) {
  if (((unsigned long long)p & 7ull) == 0)
    ff_load_slots<0>(p, nb, v);
  else
    ff_load_slots<1>(p, nb, v);
}

// pairs [.][2]: the rows (i, j <= i) of two galaxies of one field, counted like every per-galaxy array here from row 0 of the
// call; stamps [.][cs][cs][nb]; places [.][2]; sfield [.] the field of every row, fptr [.] the first row of every field; foff
// [.]: where the scratch of field fbase + k begins in `scratch`, in doubles; data: the observed fields from field f0 on;
// gram / proj [.][nb].  WEIGHTED (7s): weight, the weight fields from field f0 on, laid out like data; a pixel of band b counts
// iff 0 < W < inf, its terms are (W P_i) P_j and (W P_i) D, and every other pixel's terms are +0.0 by selection - nothing under
// a masked pixel reaches a sum.  W is read per band inside the unrolled band loop, as D is: no further band slots.  The
// unweighted instantiation never touches `weight`.
__device__ __forceinline__ bool ff_counts(double w) { return w > 0.0 && w < __longlong_as_double(0x7ff0000000000000LL); }

// (INDEXED, 7y, is a fourth flag behind the three of 7q - 7w.  It sits in the kernel and not in a body shared by two kernels: an
// inlined body changed the registers of the weighted instantiations.  The launches of 7q - 7w spell the flags they spelt - the
// header read `template <bool WEIGHTED, int Q = 0, bool GROUPED = false>`, the text tests/test_fit_flux_groups_host.py looks
// for - and compile to the code they compiled to.)
template <bool WEIGHTED, int Q = 0, bool GROUPED = false, bool INDEXED = false>
__global__ __launch_bounds__(MS_THREADS) void fitflux_gram_kernel(const int* __restrict__ pairs, const float* __restrict__ stamps,
                                                                  const int* __restrict__ places, const int* __restrict__ sfield,
                                                                  const int* __restrict__ fptr, const long long* __restrict__ foff,
                                                                  int fbase, int f0, int cs, int nb, int F,
                                                                  const double* __restrict__ data, double* __restrict__ scratch,
                                                                  double* __restrict__ gram, double* __restrict__ proj,
                                                                  const double* __restrict__ weight,
                                                                  const int* __restrict__ rtab = nullptr,
                                                                  const long long* __restrict__ gtab = nullptr, int rbase = 0,
                                                                  int sub = 0, const int* __restrict__ srow = nullptr) {
  __shared__ double s_red[MS_RED];
  const long gi = pairs[2 * (long)blockIdx.x], gj = pairs[2 * (long)blockIdx.x + 1];
  const int m = sfield[gi];
  // GROUPED (7w): the blend group of the pair in place of its field - the group's scratch, its size, the positions of the two
  // rows inside it; a pair of a group that goes through the scratch in another sub-range is left to that sub-range's launch
  const long long* gt = GROUPED ? gtab + 4 * (long)rtab[2 * (gi - rbase)] : nullptr;
  if (GROUPED && gt[3] != sub) return;         // (uniform: the whole workgroup takes one pair)
  const int row0 = GROUPED ? 0 : fptr[m];
  const int n = GROUPED ? (int)gt[2] : fptr[m + 1] - row0 + Q;   // (the row length of the scratch: Q sky terms behind the galaxies, 7t)
  const int pri = places[2 * gi], pci = places[2 * gi + 1], prj = places[2 * gj], pcj = places[2 * gj + 1];
  // the intersection of the two stamps and the field, in field pixels (the host lists a pair only where it is not empty)
  const int ra = max(max(pri, prj), 0), rz = min(min(pri, prj) + cs, F);
  const int ca = max(max(pci, pcj), 0), cz = min(min(pci, pcj) + cs, F);
  const int w = cz - ca, npix = (rz - ra) * w;
  const bool diag = gi == gj;                // (uniform: the whole workgroup takes one pair)
  // INDEXED (7y): the stamps lie where the set's passes put them, srow [.] the place of every row of the call in that store
  const float* Pi = stamps + (INDEXED ? (long)srow[gi] : gi) * cs * cs * nb;
  const float* Pj = stamps + (INDEXED ? (long)srow[gj] : gj) * cs * cs * nb;
  const double* D = data + (long)(m - f0) * F * F * nb;
  const double* W = WEIGHTED ? weight + (long)(m - f0) * F * F * nb : nullptr;
  double g[FF_BANDS], h[FF_BANDS], vi[FF_BANDS], vj[FF_BANDS];
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) g[b] = h[b] = vi[b] = vj[b] = 0.0;
  for (int e = threadIdx.x; e < npix; e += MS_THREADS) {
    const int r = ra + e / w, c = ca + e % w;
    ff_load(Pi + ((long)(r - pri) * cs + (c - pci)) * nb, nb, vi);
    const double* wp = WEIGHTED ? W + ((long)r * F + c) * nb : nullptr;
    if (diag) {
      const double* dp = D + ((long)r * F + c) * nb;
#pragma unroll
      for (int b = 0; b < FF_BANDS; ++b) {
        if (b < nb) {
          if (WEIGHTED) {
            const double wv = wp[b];
            const bool on = ff_counts(wv);
            const double wi = wv * vi[b];
            g[b] += on ? wi * vi[b] : 0.0;
            h[b] += on ? wi * dp[b] : 0.0;
          } else {
            g[b] += vi[b] * vi[b];
            h[b] += vi[b] * dp[b];
          }
        }
      }
    } else {
      ff_load(Pj + ((long)(r - prj) * cs + (c - pcj)) * nb, nb, vj);
#pragma unroll
      for (int b = 0; b < FF_BANDS; ++b) {
        if (b < nb) {
          if (WEIGHTED) {
            const double wv = wp[b];
            g[b] += ff_counts(wv) ? (wv * vi[b]) * vj[b] : 0.0;
          } else {
            g[b] += vi[b] * vj[b];
          }
        }
      }
    }
  }
  const long il = GROUPED ? rtab[2 * (gi - rbase) + 1] : gi - row0, jl = GROUPED ? rtab[2 * (gj - rbase) + 1] : gj - row0;
  double* S = scratch + (GROUPED ? gt[0] : foff[m - fbase]) + il * n + jl;
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) {
    if (b < nb) {                            // (nb and diag are uniform: every thread takes the same barriers)
      if (diag) {
        double a[2] = {g[b], h[b]};
        ms_block_sum<2>(a, s_red);
        if (threadIdx.x == 0) {
          S[(long)b * n * n] = a[0];
          gram[gi * nb + b] = a[0];
          proj[gi * nb + b] = a[1];
        }
      } else {
        double a[1] = {g[b]};
        ms_block_sum<1>(a, s_red);
        if (threadIdx.x == 0) S[(long)b * n * n] = a[0];
      }
    }
  }
}

// The weight of band b at a pixel and whether the pixel counts there; unweighted: 1.0, and every pixel counts
template <bool WEIGHTED>
__device__ __forceinline__ double ff_weight(const double* __restrict__ wp, int b, bool& on) {
  const double wv = WEIGHTED ? wp[b] : 1.0;
  on = WEIGHTED ? ff_counts(wv) : true;
  return wv;
}

// The sky basis of the bordered fit (7t) at field row or column x of a field of side F: an integer numerator, one division.
__device__ __forceinline__ double ff_basis(int x, int F) { return (double)(2 * x - F + 1) / (double)F; }

// The sums of a field that the sky terms need (7t, step 1), Q = 1: K00, c0 and the counting pixels; Q = 3: K00 K10 K11 K20
// K21 K22, c0 c1 c2 and the counting pixels - SKY_ACC(Q) doubles per band.  A streaming reduction over D (and W) in a tiling
// that depends on F alone: tile blockIdx.x % ntiles holds SKY_TILE consecutive pixels in raster order, thread t takes pixels
// t, t + 256, ... of it, consecutive lanes consecutive pixels; blockIdx.y takes SKY_GROUP bands in statically indexed slots
// (ten accumulators per band: all sixteen bands at once would not fit the registers); blockIdx.x also counts the fields of
// the sub-range, field fd0 + blockIdx.x / ntiles of `data`.  One ms_block_sum per band and half of its accumulators; thread 0
// writes the tile's partial sums to part [field][band][tile][acc].
constexpr int SKY_TILE = FF_SKY_TILE, SKY_GROUP = 4;
__host__ __device__ constexpr int SKY_ACC(int q) { return q == 1 ? 3 : 10; }

template <bool WEIGHTED, int Q>
__global__ __launch_bounds__(MS_THREADS) void fitflux_skysum_kernel(int fd0, int nb, int F, int ntiles, const double* __restrict__ data,
                                                                    const double* __restrict__ weight, double* __restrict__ part) {
  constexpr int NA = SKY_ACC(Q);
  __shared__ double s_red[MS_RED];
  const int tile = (int)(blockIdx.x % (unsigned)ntiles), b0 = (int)blockIdx.y * SKY_GROUP, fl = (int)(blockIdx.x / (unsigned)ntiles);
  const long npix = (long)F * F;
  const double* D = data + (long)(fd0 + fl) * npix * nb;
  const double* W = WEIGHTED ? weight + (long)(fd0 + fl) * npix * nb : nullptr;
  double acc[SKY_GROUP][NA];
#pragma unroll
  for (int g = 0; g < SKY_GROUP; ++g)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[g][a] = 0.0;
  const long e0 = (long)tile * SKY_TILE;
  for (int k = threadIdx.x; k < SKY_TILE; k += MS_THREADS) {
    const long e = e0 + k;
    if (e >= npix) break;
    const int r = (int)(e / F), c = (int)(e - (long)r * F);
    const double B1 = Q == 3 ? ff_basis(r, F) : 0.0, B2 = Q == 3 ? ff_basis(c, F) : 0.0;
#pragma unroll
    for (int g = 0; g < SKY_GROUP; ++g) {
      if (b0 + g < nb) {
        const double d = D[e * nb + b0 + g];
        bool on;
        const double wv = ff_weight<WEIGHTED>(WEIGHTED ? W + e * nb : nullptr, b0 + g, on);
        const double w0 = wv * 1.0;
        if constexpr (Q == 1) {
          acc[g][0] += on ? w0 * 1.0 : 0.0;
          acc[g][1] += on ? w0 * d : 0.0;
          acc[g][2] += on ? 1.0 : 0.0;
        } else {
          const double w1 = wv * B1, w2 = wv * B2;
          acc[g][0] += on ? w0 * 1.0 : 0.0;
          acc[g][1] += on ? w1 * 1.0 : 0.0;
          acc[g][2] += on ? w1 * B1 : 0.0;
          acc[g][3] += on ? w2 * 1.0 : 0.0;
          acc[g][4] += on ? w2 * B1 : 0.0;
          acc[g][5] += on ? w2 * B2 : 0.0;
          acc[g][6] += on ? w0 * d : 0.0;
          acc[g][7] += on ? w1 * d : 0.0;
          acc[g][8] += on ? w2 * d : 0.0;
          acc[g][9] += on ? 1.0 : 0.0;
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < SKY_GROUP; ++g) {
    if (b0 + g < nb) {                          // (uniform: every thread takes the same barriers)
      double* o = part + (((long)fl * nb + b0 + g) * ntiles + tile) * NA;
      if constexpr (Q == 1) {
        double a[3] = {acc[g][0], acc[g][1], acc[g][2]};
        ms_block_sum<3>(a, s_red);
        if (threadIdx.x == 0) {
          o[0] = a[0];
          o[1] = a[1];
          o[2] = a[2];
        }
      } else {
        double a[5] = {acc[g][0], acc[g][1], acc[g][2], acc[g][3], acc[g][4]};
        double c[5] = {acc[g][5], acc[g][6], acc[g][7], acc[g][8], acc[g][9]};
        ms_block_sum<5>(a, s_red);
        ms_block_sum<5>(c, s_red);
        if (threadIdx.x == 0) {
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            o[k] = a[k];
            o[5 + k] = c[k];
          }
        }
      }
    }
  }
}

// The partial sums of field fbase + blockIdx.x, band blockIdx.y, in tile order: thread t adds tiles t, t + 256, ... one after
// another, then one ms_block_sum - an order that depends on F alone.  Thread 0 writes K and c to sums [field of the sub-range]
// [nb][SKY_ACC] (the solve reads its diagonal and right-hand side there), K into the corner of the field's scratch and the
// counting pixels to npix [field of the call][nb].
template <int Q>
__global__ __launch_bounds__(MS_THREADS) void fitflux_skyreduce_kernel(const int* __restrict__ fptr, const long long* __restrict__ foff,
                                                                       int fbase, int nb, int ntiles, const double* __restrict__ part,
                                                                       double* __restrict__ scratch, double* __restrict__ sums,
                                                                       long long* __restrict__ npix) {
  constexpr int NA = SKY_ACC(Q);
  __shared__ double s_red[MS_RED];
  const int fl = (int)blockIdx.x, m = fbase + fl, b = (int)blockIdx.y;
  const int n = fptr[m + 1] - fptr[m], nt = n + Q;
  const double* p = part + ((long)fl * nb + b) * ntiles * NA;
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += MS_THREADS) {
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] += p[(long)t * NA + a];
  }
  if constexpr (Q == 1) {
    ms_block_sum<NA>(acc, s_red);
  } else {
    double a[5], c[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      a[k] = acc[k];
      c[k] = acc[5 + k];
    }
    ms_block_sum<5>(a, s_red);
    ms_block_sum<5>(c, s_red);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      acc[k] = a[k];
      acc[5 + k] = c[k];
    }
  }
  if (threadIdx.x == 0) {
    double* o = sums + ((long)fl * nb + b) * NA;
#pragma unroll
    for (int a = 0; a < NA; ++a) o[a] = acc[a];
    npix[(long)m * nb + b] = (long long)acc[NA - 1];
    double* S = scratch + foff[fl] + (long)b * nt * nt;
    int a = 0;
#pragma unroll
    for (int t = 0; t < Q; ++t)
#pragma unroll
      for (int u = 0; u <= t; ++u) S[(long)(n + t) * nt + n + u] = acc[a++];
  }
}

// E_it = sum over the pixels of galaxy r0 + blockIdx.x of (W P_i) B_t (7t, step 1; unweighted P_i B_t), into row n + t,
// column i of the field's scratch.  One workgroup per galaxy: the pixels of the clipped stamp in raster order, stride 256,
// ff_load and one ms_block_sum per band, as the diagonal path of the Gram kernel - in a kernel of its own, so that kernel
// keeps its registers.  A stamp wholly outside its field writes the empty sums.
template <bool WEIGHTED, int Q>
__global__ __launch_bounds__(MS_THREADS) void fitflux_border_kernel(int r0, const float* __restrict__ stamps, const int* __restrict__ places,
                                                                    const int* __restrict__ sfield, const int* __restrict__ fptr,
                                                                    const long long* __restrict__ foff, int fbase, int f0, int cs,
                                                                    int nb, int F, double* __restrict__ scratch,
                                                                    const double* __restrict__ weight) {
  __shared__ double s_red[MS_RED];
  const long gi = (long)r0 + blockIdx.x;
  const int m = sfield[gi];
  const int row0 = fptr[m], n = fptr[m + 1] - row0, nt = n + Q;
  const int pri = places[2 * gi], pci = places[2 * gi + 1];
  const int ra = max(pri, 0), rz = min(pri + cs, F), ca = max(pci, 0), cz = min(pci + cs, F);
  const int w = cz - ca, npix = (rz > ra && w > 0) ? (rz - ra) * w : 0;
  const float* Pi = stamps + gi * cs * cs * nb;
  const double* W = WEIGHTED ? weight + (long)(m - f0) * F * F * nb : nullptr;
  double e[FF_BANDS][Q], vi[FF_BANDS];
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) {
    vi[b] = 0.0;
#pragma unroll
    for (int t = 0; t < Q; ++t) e[b][t] = 0.0;
  }
  for (int x = threadIdx.x; x < npix; x += MS_THREADS) {
    const int r = ra + x / w, c = ca + x % w;
    ff_load(Pi + ((long)(r - pri) * cs + (c - pci)) * nb, nb, vi);
    const double* wp = WEIGHTED ? W + ((long)r * F + c) * nb : nullptr;
    const double B1 = Q == 3 ? ff_basis(r, F) : 0.0, B2 = Q == 3 ? ff_basis(c, F) : 0.0;
#pragma unroll
    for (int b = 0; b < FF_BANDS; ++b) {
      if (b < nb) {
        bool on;
        const double wv = ff_weight<WEIGHTED>(wp, b, on);
        const double wi = wv * vi[b];
        e[b][0] += on ? wi * 1.0 : 0.0;
        if constexpr (Q == 3) {
          e[b][1] += on ? wi * B1 : 0.0;
          e[b][2] += on ? wi * B2 : 0.0;
        }
      }
    }
  }
  double* S = scratch + foff[m - fbase] + (long)n * nt + (gi - row0);
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) {
    if (b < nb) {                              // (nb is uniform: every thread takes the same barriers)
      ms_block_sum<Q>(e[b], s_red);
      if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < Q; ++t) S[(long)b * nt * nt + (long)t * nt] = e[b][t];
      }
    }
  }
}

// Field fbase + blockIdx.x, band blockIdx.y.  S = its [n][n] scratch: on entry G in the lower triangle, zeros above.  W(i, j),
// j < i - the working copy, then L - lies at S[j n + i]; the diagonal in place.  LDS: the status of every galaxy and the
// right-hand side, 12 KB.
// Q > 0 is the bordered system of 7t: nt = n + Q unknowns - the galaxies, then the sky terms, whose rows of the scratch the
// border and sky-reduce kernels filled; the diagonal and right-hand side of sky term t come from skysums [field of the
// sub-range][nb][SKY_ACC(Q)].  Every step below runs on the nt unknowns; what differs for a sky term: a dropped one has
// coefficient 0.0 and leaves the right-hand sides alone (step 4 sums over the dropped GALAXIES), and its outputs go to
// sky_coef / sky_status [field][nb][Q] and sky_cov [field][nb][Q][Q], the corner of (L^-1)^T L^-1.  The sky terms come last, so
// every operation on the galaxy block is the one of Q = 0, in the same order; Q = 0 is the kernel as it was.
template <int Q, bool GROUPED = false>
__global__ __launch_bounds__(MS_THREADS) void fitflux_solve_kernel(const int* __restrict__ fptr, const long long* __restrict__ foff,
                                                                   int fbase, int nb, double min_pivot,
                                                                   double* __restrict__ scratch, const double* __restrict__ gram,
                                                                   const double* __restrict__ proj, double* __restrict__ scale,
                                                                   double* __restrict__ var, int* __restrict__ status,
                                                                   const double* __restrict__ skysums, double* __restrict__ sky_coef,
                                                                   double* __restrict__ sky_cov, int* __restrict__ sky_status,
                                                                   const int* __restrict__ grows = nullptr,
                                                                   const long long* __restrict__ gtab = nullptr) {
  __shared__ double s_y[FF_MAX_N + Q];
  __shared__ int s_st[FF_MAX_N + Q];
  // GROUPED (7w): blend group fbase + blockIdx.x in place of a field - gtab [.][4]: where its scratch begins, its first slot of
  // `grows`, its size; unknown k is row grows[first + k] of the call, the members in ascending row order
  const long long* gt = GROUPED ? gtab + 4 * (long)(fbase + (int)blockIdx.x) : nullptr;
  const int m = fbase + (int)blockIdx.x, b = (int)blockIdx.y;
  const long row0 = GROUPED ? 0 : fptr[m];
  const int ng = GROUPED ? (int)gt[2] : fptr[m + 1] - (int)row0;      // the galaxies
  const int n = ng + Q;                        // the unknowns
  if (n <= 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* S = scratch + (GROUPED ? gt[0] : foff[blockIdx.x]) + (long)b * n * n;
  const int* gr = GROUPED ? grows + gt[1] : nullptr;
  auto row = [&](int k) -> long { return GROUPED ? (long)gr[k] : row0 + k; };
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double* ks = Q > 0 ? skysums + ((long)blockIdx.x * nb + b) * SKY_ACC(Q) : nullptr;
  // G_kk as step 1 left it and the right-hand side of unknown k (sky term t: K_tt at t (t + 3) / 2 of the sums, c_t behind K)
  auto diag0 = [&](int k) -> double {
    if (Q > 0 && k >= ng) return ks[(k - ng) * (k - ng + 3) / 2];
    return gram[row(k) * nb + b];
  };
  auto rhs0 = [&](int k) -> double {
    if (Q > 0 && k >= ng) return ks[Q * (Q + 1) / 2 + (k - ng)];
    return proj[row(k) * nb + b];
  };

  // step 2 and the working copy
  for (int i = tid; i < n; i += MS_THREADS) {
    const double gii = diag0(i);
    s_st[i] = (ms_finite(gii) && gii > 0.0) ? 0 : 4;
  }
  for (int i = wave; i < n; i += MS_THREADS / 64)
    for (int j = lane; j < i; j += 64) S[(long)j * n + i] = S[(long)i * n + j];
  __syncthreads();

  // step 3: right-looking, column by column; element (i, j) of the trailing part belongs to one thread in every column
  for (int k = 0; k < n; ++k) {
    if (s_st[k] != 0) continue;              // (uniform; s_st[k] was last written behind a barrier)
    const double d = S[(long)k * n + k];
    const double gkk = diag0(k);
    if (d <= min_pivot * gkk) {              // (uniform: every thread read the same two values)
      __syncthreads();                       // everyone has read s_st[k]
      if (tid == 0) s_st[k] = 5;
      __syncthreads();
      continue;
    }
    const double lkk = __dsqrt_rn(d);
    __syncthreads();                         // everyone has read the pivot
    if (tid == 0) S[(long)k * n + k] = lkk;
    for (int i = k + 1 + tid; i < n; i += MS_THREADS)
      if (s_st[i] == 0) S[(long)k * n + i] = S[(long)k * n + i] / lkk;
    __syncthreads();
    for (int j = k + 1 + wave; j < n; j += MS_THREADS / 64) {
      if (s_st[j] != 0) continue;
      const double ljk = S[(long)k * n + j];
      for (int i = j + lane; i < n; i += 64)
        if (s_st[i] == 0) S[(long)j * n + i] = S[(long)j * n + i] - S[(long)k * n + i] * ljk;
    }
    __syncthreads();
  }

  // step 4: the right-hand side less the dropped galaxies at the network's amplitude (G as the Gram kernel left it)
  for (int i = tid; i < n; i += MS_THREADS) {
    double hp = rhs0(i);
    if (s_st[i] == 0) {
      for (int k = 0; k < ng; ++k)
        if (s_st[k] == 5) hp = hp - (k < i ? S[(long)i * n + k] : S[(long)k * n + i]);   // (G_ik lies at (max, min))
    }
    s_y[i] = hp;
  }
  __syncthreads();

  // step 5: L y = h', then L^T a = y, column-oriented: once y_k is known it leaves every later right-hand side
  for (int k = 0; k < n; ++k) {
    if (s_st[k] != 0) continue;
    const double yk = s_y[k] / S[(long)k * n + k];
    __syncthreads();                         // everyone has read s_y[k]
    if (tid == 0) s_y[k] = yk;
    for (int i = k + 1 + tid; i < n; i += MS_THREADS)
      if (s_st[i] == 0) s_y[i] = s_y[i] - S[(long)k * n + i] * yk;
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    if (s_st[k] != 0) continue;
    const double ak = s_y[k] / S[(long)k * n + k];
    __syncthreads();
    if (tid == 0) s_y[k] = ak;
    for (int i = tid; i < k; i += MS_THREADS)
      if (s_st[i] == 0) s_y[i] = s_y[i] - S[(long)i * n + k] * ak;
    __syncthreads();
  }

  // column i of X = L^-1, one thread per column, into the strict lower triangle (X(r, i) at S[r n + i]): X(i, i) = 1 / L_ii,
  // X(r, i) = -(sum_{i <= c < r} L_rc X(c, i)) / L_rr, c ascending.  The loops run over the same (r, c) in every lane, so
  // the loads of L are uniform and those of X are contiguous over the lanes.
  for (int i0 = 0; i0 < n; i0 += MS_THREADS) {
    const int i = i0 + tid;
    const bool on = i < n && s_st[i] == 0;
    double xi = 0.0, acc = 0.0;
    if (on) {
      xi = 1.0 / S[(long)i * n + i];
      acc = xi * xi;
    }
    for (int r = i0 + 1; r < n; ++r) {
      if (s_st[r] != 0) continue;            // (uniform)
      double sum = 0.0;
      if (on && r > i) sum = S[(long)i * n + r] * xi;
      for (int c = i0 + 1; c < r; ++c) {
        if (s_st[c] != 0) continue;
        if (on && c > i) sum = sum + S[(long)c * n + r] * S[(long)c * n + i];
      }
      if (on && r > i) {
        const double x = -sum / S[(long)r * n + r];
        S[(long)r * n + i] = x;
        acc = acc + x * x;
      }
    }
    if (i < ng) {
      const long o = row(i) * nb + b;
      const int st = s_st[i];
      scale[o] = st == 0 ? s_y[i] : st == 5 ? 1.0 : nan;
      var[o] = st == 0 ? acc : nan;
      status[o] = st;
    }
  }
  if constexpr (Q > 0) {
    // the sky terms: the corner of (L^-1)^T L^-1 from the last Q columns of X, rows ascending, in one thread
    __syncthreads();                           // the columns of X are complete
    if (tid == 0) {
      const long o = (long)m * nb + b;
      for (int t = 0; t < Q; ++t) {
        const int st = s_st[ng + t];
        sky_coef[o * Q + t] = st == 0 ? s_y[ng + t] : st == 5 ? 0.0 : nan;
        sky_status[o * Q + t] = st;
        for (int u = 0; u <= t; ++u) {
          double cv = nan;
          if (st == 0 && s_st[ng + u] == 0) {
            cv = 0.0;
            for (int r = ng + t; r < n; ++r) {
              if (s_st[r] != 0) continue;
              const double xt = r == ng + t ? 1.0 / S[(long)r * n + r] : S[(long)r * n + ng + t];
              const double xu = r == ng + u ? 1.0 / S[(long)r * n + r] : S[(long)r * n + ng + u];
              cv = cv + xt * xu;
            }
          }
          sky_cov[(o * Q + t) * Q + u] = cv;
          sky_cov[(o * Q + u) * Q + t] = cv;
        }
      }
    }
  }
}

// The non-negative fit: the same quadratic minimised subject to a_i >= 0 for the galaxies, the sky left free,
// by block principal pivoting (Kim & Park) with Murty's single exchange as the backup rule.  Field fbase + blockIdx.x, band
// blockIdx.y, on the scratch of fitflux_solve_kernel and in its place.  Iteration 1 is that kernel's steps 2 - 5, operation
// for operation: it fixes fit_status, the dropped set, h' (s_hp) and the unconstrained amplitudes (scale_free).  Every
// iteration rebuilds the working copy - the strict upper triangle from the strict lower one, which keeps G, the diagonal
// from gram / skysums -, factorises it over the kept unknowns that are not clamped (s_on; no pivot test after iteration 1: a
// pivot over a subset of the predecessors is not smaller), solves, and takes y_i = (sum_j G_ij a_j) - h'_i for every clamped
// i, j ascending over s_on, sequentially in one thread.  s_y holds a_i for the passive unknowns and y_i for the clamped
// galaxies, so V is the kept galaxies with s_y < 0.0; its size and largest member come from integer reductions in LDS, and
// every thread keeps the same exchange state (best, p).  L^-1 comes last, on the last passive set, because it overwrites G.
// LDS: 2 x 8 KB of doubles, 3 x 4 KB of flags, 2 KB of reduction.  No atomics, nothing handed between workgroups.
template <int Q>
__global__ __launch_bounds__(MS_THREADS) void fitflux_nonneg_kernel(const int* __restrict__ fptr, const long long* __restrict__ foff,
                                                                    int fbase, int nb, double min_pivot, int max_iter,
                                                                    double* __restrict__ scratch, const double* __restrict__ gram,
                                                                    const double* __restrict__ proj, double* __restrict__ scale,
                                                                    double* __restrict__ var, int* __restrict__ status,
                                                                    double* __restrict__ scale_free, int* __restrict__ clamped,
                                                                    double* __restrict__ dual, int* __restrict__ nn_iters,
                                                                    int* __restrict__ nn_status, const double* __restrict__ skysums,
                                                                    double* __restrict__ sky_coef, double* __restrict__ sky_cov,
                                                                    int* __restrict__ sky_status) {
  __shared__ double s_y[FF_MAX_N + Q];         // a_i of a passive unknown, y_i of a clamped galaxy
  __shared__ double s_hp[FF_MAX_N + Q];        // h' (step 4), fixed by iteration 1
  __shared__ int s_st[FF_MAX_N + Q];           // 0 / 4 / 5, frozen after iteration 1
  __shared__ int s_z[FF_MAX_N + Q];            // bit 0: clamped; bit 1: in V of this iteration
  __shared__ int s_on[FF_MAX_N + Q];           // kept and not clamped: part of this iteration's system
  __shared__ int s_cnt[MS_THREADS], s_max[MS_THREADS];
  const int m = fbase + (int)blockIdx.x, b = (int)blockIdx.y;
  const long row0 = fptr[m];
  const int ng = fptr[m + 1] - (int)row0;      // the galaxies
  const int n = ng + Q;                        // the unknowns
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (n <= 0) {
    if (tid == 0) nn_iters[(long)m * nb + b] = nn_status[(long)m * nb + b] = 0;
    return;
  }
  double* S = scratch + foff[blockIdx.x] + (long)b * n * n;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double* ks = Q > 0 ? skysums + ((long)blockIdx.x * nb + b) * SKY_ACC(Q) : nullptr;
  auto diag0 = [&](int k) -> double {
    if (Q > 0 && k >= ng) return ks[(k - ng) * (k - ng + 3) / 2];
    return gram[(row0 + k) * nb + b];
  };
  auto rhs0 = [&](int k) -> double {
    if (Q > 0 && k >= ng) return ks[Q * (Q + 1) / 2 + (k - ng)];
    return proj[(row0 + k) * nb + b];
  };

  // step 2
  for (int i = tid; i < n; i += MS_THREADS) {
    const double gii = diag0(i);
    s_st[i] = (ms_finite(gii) && gii > 0.0) ? 0 : 4;
    s_z[i] = 0;
  }
  int best = ng + 1, p = 3, iters = 0, nviol = 0;
  for (int t = 1;; ++t) {
    // the working copy, and who is in the system (thread i % 256 owns the flags of unknown i throughout)
    for (int i = tid; i < n; i += MS_THREADS) {
      s_on[i] = s_st[i] == 0 && !(s_z[i] & 1);
      S[(long)i * n + i] = diag0(i);
    }
    for (int i = wave; i < n; i += MS_THREADS / 64)
      for (int j = lane; j < i; j += 64) S[(long)j * n + i] = S[(long)i * n + j];
    __syncthreads();

    // step 3 over s_on, right-looking as in fitflux_solve_kernel; the pivot test and the dropping in iteration 1 alone
    for (int k = 0; k < n; ++k) {
      if (!s_on[k]) continue;                  // (uniform; s_on[k] was last written behind a barrier)
      const double d = S[(long)k * n + k];
      if (t == 1 && d <= min_pivot * diag0(k)) {
        __syncthreads();                       // everyone has read s_on[k]
        if (tid == 0) {
          s_st[k] = 5;
          s_on[k] = 0;
        }
        __syncthreads();
        continue;
      }
      const double lkk = __dsqrt_rn(d);
      __syncthreads();                         // everyone has read the pivot
      if (tid == 0) S[(long)k * n + k] = lkk;
      for (int i = k + 1 + tid; i < n; i += MS_THREADS)
        if (s_on[i]) S[(long)k * n + i] = S[(long)k * n + i] / lkk;
      __syncthreads();
      for (int j = k + 1 + wave; j < n; j += MS_THREADS / 64) {
        if (!s_on[j]) continue;
        const double ljk = S[(long)k * n + j];
        for (int i = j + lane; i < n; i += 64)
          if (s_on[i]) S[(long)j * n + i] = S[(long)j * n + i] - S[(long)k * n + i] * ljk;
      }
      __syncthreads();
    }

    // step 4, once: the dropped set is frozen
    if (t == 1) {
      for (int i = tid; i < n; i += MS_THREADS) {
        double hp = rhs0(i);
        if (s_st[i] == 0) {
          for (int k = 0; k < ng; ++k)
            if (s_st[k] == 5) hp = hp - (k < i ? S[(long)i * n + k] : S[(long)k * n + i]);   // (G_ik lies at (max, min))
        }
        s_hp[i] = hp;
      }
    }
    for (int i = tid; i < n; i += MS_THREADS) s_y[i] = s_hp[i];
    __syncthreads();

    // step 5 over s_on
    for (int k = 0; k < n; ++k) {
      if (!s_on[k]) continue;
      const double yk = s_y[k] / S[(long)k * n + k];
      __syncthreads();                         // everyone has read s_y[k]
      if (tid == 0) s_y[k] = yk;
      for (int i = k + 1 + tid; i < n; i += MS_THREADS)
        if (s_on[i]) s_y[i] = s_y[i] - S[(long)k * n + i] * yk;
      __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {
      if (!s_on[k]) continue;
      const double ak = s_y[k] / S[(long)k * n + k];
      __syncthreads();
      if (tid == 0) s_y[k] = ak;
      for (int i = tid; i < k; i += MS_THREADS)
        if (s_on[i]) s_y[i] = s_y[i] - S[(long)i * n + k] * ak;
      __syncthreads();
    }

    // the unconstrained amplitudes; the duals of the clamped galaxies; V
    int cnt = 0, mx = -1;
    for (int i = tid; i < ng; i += MS_THREADS) {
      const int st = s_st[i];
      if (t == 1) scale_free[(row0 + i) * nb + b] = st == 0 ? s_y[i] : st == 5 ? 1.0 : nan;
      if (s_z[i] & 1) {
        double sum = 0.0;
        for (int j = 0; j < n; ++j)
          if (s_on[j]) sum = sum + (j < i ? S[(long)i * n + j] : S[(long)j * n + i]) * s_y[j];
        s_y[i] = sum - s_hp[i];                // (i is not in the system: nobody reads s_y[i] in this loop)
      }
      const int v = st == 0 && s_y[i] < 0.0;
      s_z[i] = (s_z[i] & 1) | (v << 1);
      cnt += v;
      if (v) mx = i;                           // (i ascends)
    }
    s_cnt[tid] = cnt;
    s_max[tid] = mx;
    __syncthreads();
    for (int o = MS_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) {
        s_cnt[tid] += s_cnt[tid + o];
        s_max[tid] = max(s_max[tid], s_max[tid + o]);
      }
      __syncthreads();
    }
    nviol = s_cnt[0];
    mx = s_max[0];
    iters = t;
    if (nviol == 0 || t >= max_iter) break;    // (uniform)

    // the exchange: all of V while that makes progress or p allows, else its largest member alone
    bool all = true;
    if (nviol < best) {
      best = nviol;
      p = 3;
    } else if (p > 0) {
      p -= 1;
    } else {
      all = false;
    }
    for (int i = tid; i < ng; i += MS_THREADS)
      if ((s_z[i] & 2) && (all || i == mx)) s_z[i] ^= 1;
    __syncthreads();                           // everyone has read the reduction
  }
  if (tid == 0) {
    nn_iters[(long)m * nb + b] = iters;
    nn_status[(long)m * nb + b] = nviol == 0 ? 0 : 1;
  }

  // L^-1 on the last passive set, as in fitflux_solve_kernel, and the rows
  for (int i0 = 0; i0 < n; i0 += MS_THREADS) {
    const int i = i0 + tid;
    const bool on = i < n && s_on[i];
    double xi = 0.0, acc = 0.0;
    if (on) {
      xi = 1.0 / S[(long)i * n + i];
      acc = xi * xi;
    }
    for (int r = i0 + 1; r < n; ++r) {
      if (!s_on[r]) continue;                  // (uniform)
      double sum = 0.0;
      if (on && r > i) sum = S[(long)i * n + r] * xi;
      for (int c = i0 + 1; c < r; ++c) {
        if (!s_on[c]) continue;
        if (on && c > i) sum = sum + S[(long)c * n + r] * S[(long)c * n + i];
      }
      if (on && r > i) {
        const double x = -sum / S[(long)r * n + r];
        S[(long)r * n + i] = x;
        acc = acc + x * x;
      }
    }
    if (i < ng) {
      const long o = (row0 + i) * nb + b;
      const int st = s_st[i], z = s_z[i] & 1;
      scale[o] = st == 0 ? (z ? 0.0 : s_y[i]) : st == 5 ? 1.0 : nan;
      var[o] = on ? acc : nan;
      status[o] = st;
      clamped[o] = z;
      dual[o] = st == 0 ? (z ? s_y[i] : 0.0) : nan;
    }
  }
  if constexpr (Q > 0) {
    // the sky terms, never clamped: s_on is s_st == 0 for them
    __syncthreads();                           // the columns of X are complete
    if (tid == 0) {
      const long o = (long)m * nb + b;
      for (int t = 0; t < Q; ++t) {
        const int st = s_st[ng + t];
        sky_coef[o * Q + t] = st == 0 ? s_y[ng + t] : st == 5 ? 0.0 : nan;
        sky_status[o * Q + t] = st;
        for (int u = 0; u <= t; ++u) {
          double cv = nan;
          if (st == 0 && s_st[ng + u] == 0) {
            cv = 0.0;
            for (int r = ng + t; r < n; ++r) {
              if (s_st[r] != 0) continue;
              const double xt = r == ng + t ? 1.0 / S[(long)r * n + r] : S[(long)r * n + ng + t];
              const double xu = r == ng + u ? 1.0 / S[(long)r * n + r] : S[(long)r * n + ng + u];
              cv = cv + xt * xu;
            }
          }
          sky_cov[(o * Q + t) * Q + u] = cv;
          sky_cov[(o * Q + u) * Q + t] = cv;
        }
      }
    }
  }
}

// The chi-square of the refitted scene under galaxy r0 + blockIdx.x (7s, step 3), behind the solve of its sub-range.  adj_ptr
// [rows + 1] / adj [.]: the CSR adjacency of the sub-range's rows, counted from r0: the rows of the field whose clipped
// rectangle intersects the galaxy's, ascending, itself included.  Threads take the pixels of the clipped stamp in raster order,
// stride 256; per pixel M = sum a_j P_j over the neighbours that cover it and do not have status 4, sequentially in one thread,
// then r = D - M and the terms (W r) r where the pixel counts.  The neighbours' placements, amplitudes and band masks are
// staged in LDS CHI_TILE at a time (a degree of 40 is one tile: staged once, before the pixel loop), so the inner loop reads
// no global table; one ms_block_sum per band carries chi2 and the pixel count (an integer below 2^24, exact in a double).
// Q > 0 (7t): M gains sum_t s_t B_t(p) behind the neighbours, t ascending, over the sky terms of the field with sky_status 0;
// their coefficients and band masks lie in LDS beside the staged neighbours.  Q = 0 is the kernel as it was.
// INDEXED (7y): srow [.] the place of every row's stamp in `stamps`; the staged s_row then holds that place, which nothing but
// the stamp loads reads.
constexpr int CHI_TILE = 64;

template <int Q, bool INDEXED = false>
__global__ __launch_bounds__(MS_THREADS) void fitflux_chi2_kernel(const int* __restrict__ adj_ptr, const int* __restrict__ adj, int r0,
                                                                  const float* __restrict__ stamps, const int* __restrict__ places,
                                                                  const int* __restrict__ sfield, int f0, int cs, int nb, int F,
                                                                  const double* __restrict__ data, const double* __restrict__ weight,
                                                                  const double* __restrict__ scale, const int* __restrict__ status,
                                                                  double* __restrict__ chi2, int* __restrict__ npix_out,
                                                                  const double* __restrict__ sky_coef,
                                                                  const int* __restrict__ sky_status,
                                                                  const int* __restrict__ srow = nullptr) {
  __shared__ double s_red[MS_RED];
  __shared__ double s_sky[(Q > 0 ? Q : 1) * FF_BANDS];   // Q > 0: the coefficient of sky term t in band b
  __shared__ int s_skymask[Q > 0 ? Q : 1];               //        the bands in which it has sky_status 0
  __shared__ double s_a[CHI_TILE * FF_BANDS];     // the amplitude of neighbour q in band b, 0.0 where it has status 4
  __shared__ int s_row[CHI_TILE], s_pr[CHI_TILE], s_pc[CHI_TILE], s_mask[CHI_TILE];   // its row, placement, bands summed
  const long gi = (long)r0 + blockIdx.x;
  const int m = sfield[gi];
  const int pri = places[2 * gi], pci = places[2 * gi + 1];
  const int ra = max(pri, 0), rz = min(pri + cs, F), ca = max(pci, 0), cz = min(pci + cs, F);
  const int w = cz - ca, npix = (rz > ra && w > 0) ? (rz - ra) * w : 0;
  const int a0 = adj_ptr[blockIdx.x], deg = adj_ptr[blockIdx.x + 1] - a0;
  const bool once = deg <= CHI_TILE;              // (uniform, like every bound of the loops that hold a barrier)
  const double* D = data + (long)(m - f0) * F * F * nb;
  const double* W = weight + (long)(m - f0) * F * F * nb;
  const int tid = threadIdx.x;

  // neighbours t0 .. t0 + cnt - 1 of the list into LDS: thread q the table of neighbour q, then all threads the amplitudes
  auto stage = [&](int t0, int cnt) {
    if (tid < cnt) {
      const int j = adj[a0 + t0 + tid];
      int mask = 0;
      for (int b = 0; b < nb; ++b) mask |= (status[(long)j * nb + b] != 4) << b;
      s_row[tid] = INDEXED ? srow[j] : j;
      s_pr[tid] = places[2 * (long)j];
      s_pc[tid] = places[2 * (long)j + 1];
      s_mask[tid] = mask;
    }
    for (int e = tid; e < cnt * FF_BANDS; e += MS_THREADS) {
      const int q = e / FF_BANDS, b = e % FF_BANDS;
      double a = 0.0;
      if (b < nb) {
        const long o = (long)adj[a0 + t0 + q] * nb + b;
        if (status[o] != 4) a = scale[o];
      }
      s_a[e] = a;
    }
  };
  if constexpr (Q > 0) {
    if (tid < Q) {
      int mask = 0;
      for (int b = 0; b < nb; ++b) mask |= (sky_status[((long)m * nb + b) * Q + tid] == 0) << b;
      s_skymask[tid] = mask;
    }
    if (tid < Q * FF_BANDS) {
      const int t = tid / FF_BANDS, b = tid % FF_BANDS;
      s_sky[tid] = b < nb ? sky_coef[((long)m * nb + b) * Q + t] : 0.0;
    }
    __syncthreads();
  }
  if (once) {
    stage(0, deg);
    __syncthreads();
  }

  double acc[FF_BANDS], mdl[FF_BANDS], v[FF_BANDS];
  int cnt[FF_BANDS];
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) {
    acc[b] = v[b] = 0.0;
    cnt[b] = 0;
  }
  for (int e0 = 0; e0 < npix; e0 += MS_THREADS) {
    const int e = e0 + tid;
    const bool on = e < npix;
    const int r = ra + (on ? e / w : 0), c = ca + (on ? e % w : 0);
#pragma unroll
    for (int b = 0; b < FF_BANDS; ++b) mdl[b] = 0.0;
    for (int t0 = 0; t0 < deg; t0 += CHI_TILE) {
      const int tn = min(CHI_TILE, deg - t0);
      if (!once) {
        __syncthreads();                         // everyone has read the previous tile
        stage(t0, tn);
        __syncthreads();
      }
      if (on) {
        for (int q = 0; q < tn; ++q) {
          const int dr = r - s_pr[q], dc = c - s_pc[q];
          if (dr >= 0 && dr < cs && dc >= 0 && dc < cs) {
            const int mask = s_mask[q];
            ff_load(stamps + ((long)s_row[q] * cs * cs + (long)dr * cs + dc) * nb, nb, v);
#pragma unroll
            for (int b = 0; b < FF_BANDS; ++b) {
              if (b < nb && ((mask >> b) & 1)) mdl[b] = mdl[b] + s_a[q * FF_BANDS + b] * v[b];
            }
          }
        }
      }
    }
    if (Q > 0 && on) {
      const double B[3] = {1.0, ff_basis(r, F), ff_basis(c, F)};
#pragma unroll
      for (int t = 0; t < Q; ++t) {
        const int mask = s_skymask[t];
#pragma unroll
        for (int b = 0; b < FF_BANDS; ++b) {
          if (b < nb && ((mask >> b) & 1)) mdl[b] = mdl[b] + s_sky[t * FF_BANDS + b] * B[t];
        }
      }
    }
    if (on) {
      const double* dp = D + ((long)r * F + c) * nb;
      const double* wp = W + ((long)r * F + c) * nb;
#pragma unroll
      for (int b = 0; b < FF_BANDS; ++b) {
        if (b < nb) {
          const double wv = wp[b];
          const bool counts = ff_counts(wv);
          const double res = dp[b] - mdl[b];
          acc[b] += counts ? (wv * res) * res : 0.0;
          cnt[b] += counts ? 1 : 0;
        }
      }
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int b = 0; b < FF_BANDS; ++b) {
    if (b < nb) {                                // (nb is uniform: every thread takes the same barriers)
      double a[2] = {acc[b], (double)cnt[b]};
      ms_block_sum<2>(a, s_red);
      if (tid == 0) {
        chi2[gi * nb + b] = status[gi * nb + b] == 4 ? nan : a[0];
        npix_out[gi * nb + b] = (int)a[1];
      }
    }
  }
}

// The joint fit of a resident field set: the set holds the rows of its passes pass-major, the kernels above take
// a field's rows contiguously.  One 256-thread workgroup per destination row d copies row rowmap[d] of the stamp store, its
// placement and its field: cs cs nb floats, coalesced, by 8-byte copies where both addresses allow (the address decides, as in
// ff_load) and 4-byte copies otherwise.  64-bit offsets; every destination element is written by one thread.
__global__ __launch_bounds__(MS_THREADS) void fitflux_regroup_kernel(const int* __restrict__ rowmap, const float* __restrict__ src,
                                                                     const int* __restrict__ src_places,
                                                                     const int* __restrict__ src_field, int cs, int nb,
                                                                     float* __restrict__ dst, int* __restrict__ dst_places,
                                                                     int* __restrict__ dst_field) {
  const long long d = blockIdx.x, r = rowmap[d];
  const long long stamp = (long long)cs * cs * nb;
  const float* __restrict__ p = src + r * stamp;
  float* __restrict__ q = dst + d * stamp;
  const int tid = threadIdx.x;
  if ((((unsigned long long)p | (unsigned long long)q) & 7ull) == 0) {
    const long long half = stamp >> 1;
    for (long long i = tid; i < half; i += MS_THREADS)
      reinterpret_cast<float2*>(q)[i] = reinterpret_cast<const float2*>(p)[i];
    if ((stamp & 1) && tid == 0) q[stamp - 1] = p[stamp - 1];
  } else {
    for (long long i = tid; i < stamp; i += MS_THREADS) q[i] = p[i];
  }
  if (tid < 2) dst_places[2 * d + tid] = src_places[2 * r + tid];
  if (tid == 2) dst_field[d] = src_field[r];
}

// The blend groups of a field: the connected components of the graph whose edges are the pairs of galaxies whose
// stamp rectangles, clipped to the field, intersect - the test of the pair list above.  Four kernels, integers only:
//   fitgroups_count_kernel  one workgroup per row i: its threads test every row j of i's field, stride 256, and count the
//                           adjacent j <= i and the adjacent j in all; integer sums, any order gives the same number.
//   fitgroups_scan_kernel   one workgroup: the exclusive scans of both counts, 256 rows at a time with a carry.
//   fitgroups_fill_kernel   one workgroup per row i, j ascending 256 at a time: an exclusive scan of the hits gives every hit its
//                           place - an ordered compaction.  No atomics.  The hits j <= i come first, so one scan places both the
//                           pair (i, j <= i) and the entry j of row i's adjacency list: the pair list comes out sorted by i and
//                           then j, every adjacency list ascending - the lists the host built.
//   fitgroups_label_kernel  one workgroup per field: label[i] starts at i (counted from the field's first row); a sweep gives
//                           every row the minimum label of its neighbours and itself and then that label's label (pointer
//                           jumping: a sorted chain of n links takes log2 n sweeps, any chain at most n), from one array into
//                           the other, __syncthreads() between sweeps, until a sweep changes nothing.  A label is always a
//                           row of the component that is not above the row itself, so the fixed point is the component's
//                           smallest row whatever the order of the threads.
__device__ __forceinline__ bool fg_adjacent(int pri, int pci, int prj, int pcj, int cs, int F) {
  const int ra = max(max(pri, prj), 0), rz = min(min(pri, prj) + cs, F);
  const int ca = max(max(pci, pcj), 0), cz = min(min(pci, pcj) + cs, F);
  return rz > ra && cz > ca;
}

// the exclusive prefix sum of v over the workgroup in thread order and the workgroup's total (s_w: one int per wave)
__device__ __forceinline__ int fg_block_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(x, o, 64);
    if (lane >= o) x += t;
  }
  __syncthreads();                           // s_w of the previous call has been read by everyone
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int k = 0; k < MS_THREADS / 64; ++k) base += k < wave ? s_w[k] : 0;
  total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  return base + x - v;
}

// rows r0 + blockIdx.x; cnt [2][nr]: the adjacent rows j <= i, then the adjacent rows in all
__global__ __launch_bounds__(MS_THREADS) void fitgroups_count_kernel(int r0, int nr, const int* __restrict__ places,
                                                                     const int* __restrict__ sfield, const int* __restrict__ fptr,
                                                                     int cs, int F, int* __restrict__ cnt) {
  __shared__ int s_w[MS_THREADS / 64];
  const int gi = r0 + (int)blockIdx.x, m = sfield[gi];
  const int ja = fptr[m], jz = fptr[m + 1];
  const int pri = places[2 * (long)gi], pci = places[2 * (long)gi + 1];
  int le = 0, all = 0;
  for (int j = ja + (int)threadIdx.x; j < jz; j += MS_THREADS) {
    const int hit = fg_adjacent(pri, pci, places[2 * (long)j], places[2 * (long)j + 1], cs, F) ? 1 : 0;
    all += hit;
    le += j <= gi ? hit : 0;
  }
  int tle, tall;
  fg_block_scan(le, s_w, tle);
  fg_block_scan(all, s_w, tall);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = tle;
    cnt[(long)nr + blockIdx.x] = tall;
  }
}

// ptr [2][nr + 1]: the exclusive scans of cnt [2][nr], the totals at [nr]
__global__ __launch_bounds__(MS_THREADS) void fitgroups_scan_kernel(int nr, const int* __restrict__ cnt, int* __restrict__ ptr) {
  __shared__ int s_w[MS_THREADS / 64];
  for (int a = 0; a < 2; ++a) {
    const int* c = cnt + (long)a * nr;
    int* p = ptr + (long)a * (nr + 1);
    int carry = 0;
    for (int i0 = 0; i0 < nr; i0 += MS_THREADS) {   // (uniform: every thread takes the same barriers)
      const int i = i0 + (int)threadIdx.x;
      const int v = i < nr ? c[i] : 0;
      int total;
      const int x = fg_block_scan(v, s_w, total);
      if (i < nr) p[i] = carry + x;
      carry += total;
    }
    if (threadIdx.x == 0) p[nr] = carry;
  }
}

// pairs [.][2] and adj [.] from ptr; nothing is written past the places the scan gave row i
__global__ __launch_bounds__(MS_THREADS) void fitgroups_fill_kernel(int r0, int nr, const int* __restrict__ places,
                                                                    const int* __restrict__ sfield, const int* __restrict__ fptr,
                                                                    int cs, int F, const int* __restrict__ ptr,
                                                                    int* __restrict__ pairs, int* __restrict__ adj) {
  __shared__ int s_w[MS_THREADS / 64];
  const int gi = r0 + (int)blockIdx.x, m = sfield[gi];
  const int ja = fptr[m], jz = fptr[m + 1];
  const int pri = places[2 * (long)gi], pci = places[2 * (long)gi + 1];
  const int pl = ptr[blockIdx.x], plz = ptr[blockIdx.x + 1];
  const int pa = ptr[(long)nr + 1 + blockIdx.x], paz = ptr[(long)nr + 2 + blockIdx.x];
  int base = 0;
  for (int j0 = ja; j0 < jz; j0 += MS_THREADS) {    // (uniform)
    const int j = j0 + (int)threadIdx.x;
    const int hit = (j < jz && fg_adjacent(pri, pci, places[2 * (long)j], places[2 * (long)j + 1], cs, F)) ? 1 : 0;
    int total;
    const int pos = base + fg_block_scan(hit, s_w, total);
    if (hit) {
      if (pa + pos < paz) adj[pa + pos] = j;
      if (j <= gi && pl + pos < plz) {
        pairs[2 * (long)(pl + pos)] = gi;
        pairs[2 * (long)(pl + pos) + 1] = j;
      }
    }
    base += total;
  }
}

// field fa + blockIdx.x; adj_ptr [nr + 1] / adj: the adjacency of rows r0 .., the entries rows of the call; lab [2][nr] the two
// label arrays, out [nr] the labels, counted from the field's first row
__global__ __launch_bounds__(MS_THREADS) void fitgroups_label_kernel(int r0, int nr, int fa, const int* __restrict__ fptr,
                                                                     const int* __restrict__ adj_ptr, const int* __restrict__ adj,
                                                                     int* lab, int* __restrict__ out) {
  __shared__ int s_changed;
  const int m = fa + (int)blockIdx.x;
  const int row0 = fptr[m], n = fptr[m + 1] - row0;
  const int l0 = row0 - r0;                  // the field's first row in the arrays of this launch
  int* A = lab + l0;
  int* B = lab + (long)nr + l0;
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += MS_THREADS) A[i] = i;
  if (tid == 0) s_changed = 0;
  __syncthreads();
  for (;;) {
    int changed = 0;
    for (int i = tid; i < n; i += MS_THREADS) {
      const int old = A[i];
      int l = old;
      for (int e = adj_ptr[l0 + i]; e < adj_ptr[l0 + i + 1]; ++e) l = min(l, A[adj[e] - row0]);
      l = A[l];
      B[i] = l;
      changed |= l != old;
    }
    if (changed) s_changed = 1;              // (every writer writes the same value)
    __syncthreads();
    const bool again = s_changed != 0;       // (uniform)
    __syncthreads();                         // everyone has read the flag
    if (tid == 0) s_changed = 0;
    __syncthreads();                         // the flag is clear before the next sweep sets it
    int* t = A;
    A = B;
    B = t;
    if (!again) break;
  }
  for (int i = tid; i < n; i += MS_THREADS) out[l0 + i] = A[i];
}
}  // namespace

int launch_fitflux_regroup(const int* rowmap_dev, const float* src, const int* src_places, const int* src_field, int64_t n, int cs,
                           int nb, float* dst, int* dst_places, int* dst_field, hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(fitflux_regroup_kernel, dim3((unsigned)n), dim3(MS_THREADS), 0, s, rowmap_dev, src, src_places, src_field, cs,
                     nb, dst, dst_places, dst_field);
  DV_HIP(hipGetLastError());
  return OK;
}

// the refusals that need no table, before any GPU work
int fitflux_check(const char* who, int cs, int nb, int F, const FitFluxParams& p) {
  if (cs < 1 || cs > 4096 || nb < 1 || nb > FF_BANDS) {
    set_error("%s: stamps of %d pixels and %d bands; the flux fit takes 1 .. 4096 pixels and 1 .. %d bands", who, cs, nb, FF_BANDS);
    return E_INVALID;
  }
  if (F < 1 || F > 32768) {
    set_error("%s: fields of %d pixels, 1 .. 32768 are taken", who, F);
    return E_INVALID;
  }
  if (!(p.min_pivot > 0.0 && p.min_pivot < 1.0)) {
    set_error("%s: min_pivot must lie strictly between 0 and 1 (got %g)", who, p.min_pivot);
    return E_INVALID;
  }
  if (p.scratch_bytes < 1) {
    set_error("%s: scratch_bytes must be at least 1 (got %ld)", who, (long)p.scratch_bytes);
    return E_INVALID;
  }
  return OK;
}

int fitflux_rows_check(const char* who, const FitFluxRows& o, int64_t n, bool weighted) {
  if (n > 0 && (!o.scale || !o.var || !o.gram || !o.proj || !o.status)) {
    set_error("%s: fit_scale, fit_var, fit_gram, fit_proj and fit_status must all be given", who);
    return E_INVALID;
  }
  if (weighted && n > 0 && (!o.chi2 || !o.npix)) {
    set_error("%s: fit_chi2 and fit_npix must all be given", who);
    return E_INVALID;
  }
  return OK;
}

// the two refusals by field (field_ptr has passed the caller's checks) and what the fields need: the doubles of dense scratch
// and the pair entries of the largest sub-range that goes through the scratch at once
// the refusals of the sky calls (7t) that need no table: the order, the sky outputs, and chi-square outputs that do not match
// the weights
int fitflux_sky_check(const char* who, int sky_order, const FitFluxSky& o, const FitFluxRows& rows, bool weighted) {
  if (sky_order != 0 && sky_order != 1) {
    set_error("%s: sky_order must be 0 (a constant) or 1 (a plane), got %d", who, sky_order);
    return E_INVALID;
  }
  if (!o.coef || !o.cov || !o.status || !o.npix) {
    set_error("%s: sky_coef, sky_cov, sky_status and sky_npix must all be given", who);
    return E_INVALID;
  }
  if (!weighted && (rows.chi2 || rows.npix)) {
    set_error("%s: fit_chi2 and fit_npix are the outputs of the weighted fit: without weight_fields both must be NULL", who);
    return E_INVALID;
  }
  if (weighted && (!rows.chi2 || !rows.npix)) {
    set_error("%s: fit_chi2 and fit_npix must all be given", who);
    return E_INVALID;
  }
  return OK;
}

int fitflux_nonneg_check(const char* who, const FitFluxNonneg& nn, const FitFluxRows& rows, int64_t n, const FitFluxSky& sky,
                         bool weighted) {
  if (nn.max_iter < 1) {
    set_error("%s: max_iter must be at least 1 (got %d)", who, nn.max_iter);
    return E_INVALID;
  }
  if (!nn.iters || !nn.status || (n > 0 && (!rows.scale_free || !rows.clamped || !rows.dual))) {
    set_error("%s: fit_scale_free, fit_clamped, fit_dual, nonneg_iters and nonneg_status must all be given", who);
    return E_INVALID;
  }
  if (sky.q == 0) {
    if (sky.coef || sky.cov || sky.status || sky.npix) {
      set_error("%s: sky_order -1 fits no sky: sky_coef, sky_cov, sky_status and sky_npix must all be NULL", who);
      return E_INVALID;
    }
    if (!weighted && (rows.chi2 || rows.npix)) {
      set_error("%s: fit_chi2 and fit_npix are the outputs of the weighted fit: without weight_fields both must be NULL", who);
      return E_INVALID;
    }
  }
  return OK;
}

int fitflux_plan(const char* who, const int64_t* field_ptr, int M, int nb, const FitFluxParams& p, FitFluxPlan* plan, int sky_order,
                 int F) {
  size_t total = 0, pairs = 0;
  const size_t q = sky_order < 0 ? 0 : (size_t)fitflux_sky_q(sky_order);
  for (int f = 0; f < M; ++f) {
    const int64_t n = field_ptr[f + 1] - field_ptr[f];
    if (n > FF_MAX_N) {
      set_error("%s: field %d has %ld galaxies, the dense fit takes at most %d per field", who, f, (long)n, FF_MAX_N);
      return E_INVALID;
    }
    const size_t need = (size_t)nb * (n + q) * (n + q) * sizeof(double);
    if (need > (size_t)p.scratch_bytes) {
      if (q)
        set_error("%s: field %d has %ld galaxies and %zu sky terms: its bordered matrices need %zu bytes of scratch (bands x "
                  "(n + q) x (n + q) doubles), scratch_bytes is %ld", who, f, (long)n, q, need, (long)p.scratch_bytes);
      else
        set_error("%s: field %d has %ld galaxies: its Gram matrices need %zu bytes of scratch (bands x n x n doubles), "
                  "scratch_bytes is %ld", who, f, (long)n, need, (long)p.scratch_bytes);
      return E_INVALID;
    }
    total += need / sizeof(double);
    pairs += (size_t)n * (n + 1) / 2;
  }
  const size_t cap = std::min(total, (size_t)p.scratch_bytes / sizeof(double));
  const size_t rows = (size_t)(M > 0 ? field_ptr[M] - field_ptr[0] : 0);
  plan->scratch_elems = cap;
  plan->rows = rows;
  plan->pair_cap = std::min(pairs, (cap / nb + rows) / 2 + 1);   // sum n (n + 1) / 2 over fields with sum nb n^2 <= cap
  plan->q = (int)q;
  plan->sky_part = q ? (size_t)nb * fitflux_sky_tiles(F) * fitflux_sky_acc((int)q) : 0;
  return OK;
}

int FitFluxWork::alloc(const FitFluxPlan& plan, int64_t max_fields, bool weighted) {
  cap_elems = plan.scratch_elems;
  q = plan.q;
  if (q) {
    const size_t nf = (size_t)std::max<int64_t>(max_fields, 1);
    DV_TRY(sky_part.alloc(nf * plan.sky_part));
    DV_TRY(sky_sums.alloc(nf * FF_BANDS * fitflux_sky_acc(q)));
  }
  DV_TRY(scratch.alloc(plan.scratch_elems));
  DV_TRY(pairs.alloc(2 * plan.pair_cap));
  if (weighted) {                                      // the adjacency: every pair once or twice, a pointer per row and one more
    adj_cap = std::max<size_t>(2 * plan.pair_cap, 1);
    adj_ptr_cap = plan.rows + 1;
    DV_TRY(adj.alloc(adj_cap));
    DV_TRY(adj_ptr.alloc(adj_ptr_cap));
  }
  return foff.alloc((size_t)std::max<int64_t>(max_fields, 1));
}

void fitflux_columns(Rows& r, FitFluxRows& dev, const FitFluxRows& host, int nb, bool weighted, bool nonneg) {
  r.add(dev.scale, host.scale, nb);
  r.add(dev.var, host.var, nb);
  r.add(dev.gram, host.gram, nb);
  r.add(dev.proj, host.proj, nb);
  r.add(dev.status, host.status, nb);
  if (weighted) {
    r.add(dev.chi2, host.chi2, nb);
    r.add(dev.npix, host.npix, nb);
  }
  if (nonneg) {
    r.add(dev.scale_free, host.scale_free, nb);
    r.add(dev.clamped, host.clamped, nb);
    r.add(dev.dual, host.dual, nb);
  }
}

int FitFluxFieldOut::alloc(int q, const FitFluxNonneg& nn, size_t fields, int nb) {
  const size_t e = fields * nb;
  if (q) {
    DV_TRY(coef.alloc(e * q));
    DV_TRY(cov.alloc(e * q * q));
    DV_TRY(status.alloc(e * q));
    DV_TRY(npix.alloc(e));
    sky = FitFluxSky{q, coef.get(), cov.get(), status.get(), npix.get()};
  }
  if (nn.on) {
    DV_TRY(iters.alloc(e));
    DV_TRY(nn_status.alloc(e));
    nonneg = FitFluxNonneg{true, nn.max_iter, iters.get(), nn_status.get()};
  }
  return OK;
}

int FitFluxFieldOut::download(const FitFluxSky& sky_h, const FitFluxNonneg& nn_h, size_t host_f0, size_t dev_f0, size_t nf, int nb,
                              hipStream_t s) const {
  const size_t q = (size_t)sky.q, h = host_f0 * nb, d = dev_f0 * nb, e = nf * nb;
  if (nonneg.on) {
    DV_HIP(hipMemcpyAsync(nn_h.iters + h, nonneg.iters + d, e * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(nn_h.status + h, nonneg.status + d, e * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  if (q) {
    DV_HIP(hipMemcpyAsync(sky_h.coef + h * q, sky.coef + d * q, e * q * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(sky_h.cov + h * q * q, sky.cov + d * q * q, e * q * q * sizeof(double), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(sky_h.status + h * q, sky.status + d * q, e * q * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(sky_h.npix + h, sky.npix + d, e * sizeof(long long), hipMemcpyDeviceToHost, s));
  }
  return OK;
}

namespace {
// The kernel templates of the fit are picked by whether it is weighted and by its sky terms q (0, 1 or 3): fn(wt, qc) is called
// with both as compile-time constants (std::bool_constant, std::integral_constant<int>).  A combination a call site does not
// build is left out there with `if constexpr`: nothing is instantiated for it.
template <typename Fn>
void fit_variant(bool weighted, int q, Fn&& fn) {
  auto with_q = [&](auto wt) {
    if (q == 0) fn(wt, std::integral_constant<int, 0>{});
    else if (q == 1) fn(wt, std::integral_constant<int, 1>{});
    else fn(wt, std::integral_constant<int, 3>{});
  };
  if (weighted) with_q(std::true_type{});
  else with_q(std::false_type{});
}
}  // namespace

// The complete fields fa .. fz of the view v.  The fields go through the dense scratch in sub-ranges whose Gram matrices fit it;
// the split changes no bit, a field's rows depend on nothing but the field.  Returns with the stream idle: the host tables of a
// sub-range are rebuilt for the next.  solve false: step 1 alone - the scratch keeps G of the last sub-range, gram and proj are
// written, the other rows are not touched.
int launch_fit_flux(const FieldStamps& v, const int32_t* places_h, const int* fptr_h, int fa, int fz, const FitFluxParams& p,
                    FitFluxWork& w, const FitFluxRows& rows, const FitFluxSky& sky, const FitFluxNonneg& nn, bool solve,
                    hipStream_t s) {
  const int cs = v.cs, nb = v.nb, F = v.F;
  const bool chi = v.weight && solve;                  // the chi-square of the weighted fit, behind the solve
  const int q = sky.q;                                 // the sky terms of every field (7t), 0: none
  const int ntiles = q ? (int)fitflux_sky_tiles(F) : 0;
  if (q != w.q) {                                      // (cannot happen: the plan that sized the work carries q)
    set_error("flux fit: %d sky terms asked of a work area planned for %d", q, w.q);
    return E_STATE;
  }
  for (int f = fa; f <= fz;) {
    w.foff_h.clear();
    w.pairs_h.clear();
    if (chi) w.adj_ptr_h.assign(1, 0);                 // degrees first (entry k + 1: row k of the sub-range), offsets below
    size_t used = 0;
    int g = f;
    for (; g <= fz; ++g) {
      const int row0 = fptr_h[g], n = fptr_h[g + 1] - row0;
      const size_t need = (size_t)nb * (n + q) * (n + q);
      if (used + need > w.cap_elems) break;          // (one field fits: fitflux_plan has refused the others)
      w.foff_h.push_back((long long)used);
      used += need;
      if (chi) w.adj_ptr_h.resize(w.adj_ptr_h.size() + (size_t)n, 0);
      int* deg = chi ? w.adj_ptr_h.data() + (row0 - fptr_h[f]) + 1 : nullptr;
      for (int i = 0; i < n; ++i) {
        const int pri = places_h[2 * (size_t)(row0 + i)], pci = places_h[2 * (size_t)(row0 + i) + 1];
        for (int j = 0; j <= i; ++j) {
          const int prj = places_h[2 * (size_t)(row0 + j)], pcj = places_h[2 * (size_t)(row0 + j) + 1];
          const int ra = std::max(std::max(pri, prj), 0), rz = std::min(std::min(pri, prj) + cs, F);
          const int ca = std::max(std::max(pci, pcj), 0), cz = std::min(std::min(pci, pcj) + cs, F);
          if (rz > ra && cz > ca) {
            w.pairs_h.push_back(row0 + i);
            w.pairs_h.push_back(row0 + j);
            if (chi) {
              ++deg[i];
              if (j != i) ++deg[j];
            }
          }
        }
      }
    }
    if (g == f) {                                      // (cannot happen behind fitflux_plan)
      set_error("flux fit: field %d does not fit the scratch", f);
      return E_STATE;
    }
    const int r0 = fptr_h[f], r1 = fptr_h[g];
    const size_t npairs = w.pairs_h.size() / 2;
    if (nn.on && solve) {                              // (a sub-range that launches nothing: no unknowns, no factorisation)
      DV_HIP(hipMemsetAsync(nn.iters + (size_t)f * nb, 0, (size_t)(g - f) * nb * sizeof(int), s));
      DV_HIP(hipMemsetAsync(nn.status + (size_t)f * nb, 0, (size_t)(g - f) * nb * sizeof(int), s));
    }
    if (r1 > r0 || q) {                                // (a field without galaxies still has its sky)
      DV_TRY(w.pairs.ensure(w.pairs_h.size()));
      DV_TRY(w.foff.ensure(w.foff_h.size()));
      DV_HIP(hipMemcpyAsync(w.foff, w.foff_h.data(), w.foff_h.size() * sizeof(long long), hipMemcpyHostToDevice, s));
      DV_HIP(hipMemsetAsync(w.scratch, 0, used * sizeof(double), s));
      // (a stamp wholly outside its field has no pair: its G_ii and h_i are the empty sums)
      if (r1 > r0) {
        DV_HIP(hipMemsetAsync(rows.gram + (size_t)r0 * nb, 0, (size_t)(r1 - r0) * nb * sizeof(double), s));
        DV_HIP(hipMemsetAsync(rows.proj + (size_t)r0 * nb, 0, (size_t)(r1 - r0) * nb * sizeof(double), s));
      }
      if (npairs > 0) {
        DV_HIP(hipMemcpyAsync(w.pairs, w.pairs_h.data(), w.pairs_h.size() * sizeof(int), hipMemcpyHostToDevice, s));
        fit_variant(v.weight != nullptr, q, [&](auto wt, auto qc) {
          hipLaunchKernelGGL((fitflux_gram_kernel<decltype(wt)::value, decltype(qc)::value>), dim3((unsigned)npairs), dim3(MS_THREADS), 0, s,
                             w.pairs.get(), v.stamps, v.places, v.sfield, v.fptr, w.foff.get(), f, v.f0, cs, nb, F, v.data,
                             w.scratch.get(), rows.gram, rows.proj, v.weight);
        });
        DV_HIP(hipGetLastError());
      }
      if (q) {
        // the border E (one workgroup per galaxy), then the field sums: per-tile partials, then K, c and the counting pixels
        const unsigned nf = (unsigned)(g - f), ngrp = (unsigned)((nb + SKY_GROUP - 1) / SKY_GROUP);
        if ((size_t)ntiles * nf > 0x7fffffffu) {
          set_error("flux fit: %u fields of %d tiles exceed the grid of the field sums", nf, ntiles);
          return E_INVALID;
        }
        fit_variant(v.weight != nullptr, q, [&](auto wt, auto qc) {
          constexpr bool WT = decltype(wt)::value;
          constexpr int Q = decltype(qc)::value;
          if constexpr (Q != 0) {
            if (r1 > r0)
              hipLaunchKernelGGL((fitflux_border_kernel<WT, Q>), dim3((unsigned)(r1 - r0)), dim3(MS_THREADS), 0, s, r0, v.stamps,
                                 v.places, v.sfield, v.fptr, w.foff.get(), f, v.f0, cs, nb, F, w.scratch.get(), v.weight);
            hipLaunchKernelGGL((fitflux_skysum_kernel<WT, Q>), dim3((unsigned)ntiles * nf, ngrp), dim3(MS_THREADS), 0, s, f - v.f0,
                               nb, F, ntiles, v.data, v.weight, w.sky_part.get());
            hipLaunchKernelGGL((fitflux_skyreduce_kernel<Q>), dim3(nf, (unsigned)nb), dim3(MS_THREADS), 0, s, v.fptr, w.foff.get(),
                               f, nb, ntiles, w.sky_part.get(), w.scratch.get(), w.sky_sums.get(), sky.npix);
          }
        });
        DV_HIP(hipGetLastError());
      }
      if (solve) {
        fit_variant(false, q, [&](auto, auto qc) {     // (the solvers are the same with weights and without)
          constexpr int Q = decltype(qc)::value;
          if (nn.on)                                  // (7u: in place of the solve, on the same scratch)
            hipLaunchKernelGGL((fitflux_nonneg_kernel<Q>), dim3((unsigned)(g - f), (unsigned)nb), dim3(MS_THREADS), 0, s, v.fptr,
                               w.foff.get(), f, nb, p.min_pivot, nn.max_iter, w.scratch.get(), rows.gram, rows.proj, rows.scale,
                               rows.var, rows.status, rows.scale_free, rows.clamped, rows.dual, nn.iters, nn.status,
                               (const double*)w.sky_sums.get(), sky.coef, sky.cov, sky.status);
          else
            hipLaunchKernelGGL((fitflux_solve_kernel<Q>), dim3((unsigned)(g - f), (unsigned)nb), dim3(MS_THREADS), 0, s, v.fptr,
                               w.foff.get(), f, nb, p.min_pivot, w.scratch.get(), rows.gram, rows.proj, rows.scale, rows.var,
                               rows.status, (const double*)w.sky_sums.get(), sky.coef, sky.cov, sky.status);
        });
        DV_HIP(hipGetLastError());
      }
      if (chi) {
        // the pair list is sorted by (i, j <= i): row k takes its earlier neighbours and itself while i = k, the later ones
        // as i goes on - every list comes out ascending
        const size_t nr = (size_t)(r1 - r0);
        for (size_t k = 0; k < nr; ++k) w.adj_ptr_h[k + 1] += w.adj_ptr_h[k];
        w.adj_h.resize((size_t)w.adj_ptr_h[nr]);
        w.adj_at_h.assign(w.adj_ptr_h.begin(), w.adj_ptr_h.end() - 1);
        for (size_t q = 0; q < npairs; ++q) {
          const int i = w.pairs_h[2 * q], j = w.pairs_h[2 * q + 1];
          w.adj_h[(size_t)w.adj_at_h[i - r0]++] = j;
          if (j != i) w.adj_h[(size_t)w.adj_at_h[j - r0]++] = i;
        }
        if (nr + 1 > w.adj_ptr_cap || w.adj_h.size() > w.adj_cap) {   // (cannot happen behind fitflux_plan: at most twice the pairs)
          set_error("flux fit: the adjacency of fields %d .. %d (%zu rows, %zu entries) exceeds what the plan allocated", f, g - 1,
                    nr, w.adj_h.size());
          return E_STATE;
        }
        DV_HIP(hipMemcpyAsync(w.adj_ptr, w.adj_ptr_h.data(), (nr + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (!w.adj_h.empty())
          DV_HIP(hipMemcpyAsync(w.adj, w.adj_h.data(), w.adj_h.size() * sizeof(int), hipMemcpyHostToDevice, s));
        if (nr > 0)
          fit_variant(true, q, [&](auto, auto qc) {
            hipLaunchKernelGGL((fitflux_chi2_kernel<decltype(qc)::value>), dim3((unsigned)nr), dim3(MS_THREADS), 0, s,
                               w.adj_ptr.get(), w.adj.get(), r0, v.stamps, v.places, v.sfield, v.f0, cs, nb, F, v.data, v.weight,
                               (const double*)rows.scale, (const int*)rows.status, rows.chi2, rows.npix, (const double*)sky.coef,
                               (const int*)sky.status);
          });
        DV_HIP(hipGetLastError());
      }
      DV_HIP(hipStreamSynchronize(s));
    }
    f = g;
  }
  return OK;
}

// host arrays in, host rows out, whole fields at a time (walk_whole_fields): beside the dense scratch, the stamps, tables, rows
// and per-field outputs of as many consecutive fields as half of free device memory holds
int scene_fit_flux(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                   const double* data_h, int M, int F, const FitFluxOut& rq, int device, hipStream_t s) {
  const char* who = rq.who;
  const bool weighted = rq.weights != nullptr;
  const bool with_sky = rq.sky.q != 0;                 // (the sky calls set q to a non-zero value before the order is checked)
  DV_TRY(fitflux_check(who, cs, nb, F, rq.par));
  if (with_sky) DV_TRY(fitflux_sky_check(who, rq.sky_order, rq.sky, rq.rows, weighted));
  if (rq.nonneg.on) DV_TRY(fitflux_nonneg_check(who, rq.nonneg, rq.rows, N, rq.sky, weighted));
  const int q = with_sky ? fitflux_sky_q(rq.sky_order) : 0;
  if (N < 0 || M < 0 || !field_ptr || ((N > 0 || (q && M > 0)) && !data_h) || (N > 0 && (!stamps_h || !places_h))) {
    set_error("%s: stamps, places, field_ptr and data_fields must all be given", who);
    return E_INVALID;
  }
  DV_TRY(fitflux_rows_check(who, rq.rows, N, weighted));
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, nullptr, nullptr));   // (the walker builds its own tables)
  FitFluxPlan plan;
  DV_TRY(fitflux_plan(who, field_ptr, M, nb, rq.par, &plan, with_sky ? rq.sky_order : -1, F));
  if (rq.nonneg.on && M > 0) {                         // (a field without unknowns: no factorisation, converged)
    std::fill(rq.nonneg.iters, rq.nonneg.iters + (size_t)M * nb, 0);
    std::fill(rq.nonneg.status, rq.nonneg.status + (size_t)M * nb, 0);
  }
  if (N == 0 && !(q && M > 0)) return OK;
  FieldStamps v{};
  v.cs = cs, v.nb = nb, v.F = F;
  FitFluxRows d{};
  Rows in, out;
  in.add(v.stamps, stamps_h, (size_t)cs * cs * nb);
  in.add(v.places, places_h, 2);
  fitflux_columns(out, d, rq.rows, nb, weighted, rq.nonneg.on);
  // beside the walker's: per field its scratch offset, the sums of its sky and its outputs; once, the scratch and the lists
  WholeFields f{nullptr, data_h, rq.weights, 0,
                sizeof(long long) + FitFluxWork::sky_field_bytes(plan) + FitFluxFieldOut::bytes(q, rq.nonneg.on, 1, nb),
                FitFluxWork::fixed_bytes(plan, weighted), q != 0};
  DV_HIP(hipSetDevice(device));
  FitFluxWork work;
  FitFluxFieldOut fout;
  return walk_whole_fields(who, M, field_ptr, N, f, v, in, out, s, [&](const FieldStamps& run, int fa, int nf, int64_t r0,
                                                                         const int* fptr_h) {
    if (!work.scratch) {                               // (sized by the largest run)
      DV_TRY(work.alloc(plan, (int64_t)f.max_fields, weighted));
      DV_TRY(fout.alloc(q, rq.nonneg, f.max_fields, nb));
    }
    DV_TRY(launch_fit_flux(run, places_h ? places_h + (size_t)r0 * 2 : nullptr, fptr_h, 0, nf - 1, rq.par, work, d, fout.sky,
                           fout.nonneg, true, s));
    return fout.download(rq.sky, rq.nonneg, (size_t)fa, 0, (size_t)nf, nb, s);   // the per-field outputs, with the rows
  });
}


// The fit by blend groups of the complete fields fa .. fz (7w).  Neighbour listing and labelling on the GPU; the host downloads
// the two totals and then the labels, 4 bytes per galaxy, and does the O(N) grouping: the groups of a field ordered by their
// smallest row, the members in ascending row order, fit_group / fit_group_size, the refusals, and the cut into sub-ranges of
// consecutive groups whose sum nb n_g^2 doubles fit the scratch.  One upload of the group tables serves every sub-range: a
// group's scratch offset and the number of its sub-range are part of its table entry.  The pair list is sorted by row, not by
// group, so every sub-range launches the Gram kernel over the whole list and a workgroup whose group belongs to another
// sub-range returns at once; with the default scratch there is one sub-range.  The chi-square runs once, behind the last solve,
// on the adjacency the fill kernel wrote.
int launch_fit_flux_groups(const char* who, const FieldStamps& v, const int* fptr_h, int fa, int fz, int field_base,
                           const FitFluxParams& p, FitGroupsWork& w, const FitFluxRows& rows, int32_t* group_h, int32_t* gsize_h,
                           FitGroupsLists* lists, hipStream_t s) {
  const int cs = v.cs, nb = v.nb, F = v.F;
  const int r0 = fptr_h[fa], r1 = fptr_h[fz + 1], nr = r1 - r0, nf = fz - fa + 1;
  if (nr <= 0) return OK;
  StreamDrain drain(s);                                // (a refusal or a failure below leaves the stream idle)
  DV_TRY(w.cnt.ensure(2 * (size_t)nr));
  DV_TRY(w.ptr.ensure(2 * ((size_t)nr + 1)));
  DV_TRY(w.lab.ensure(2 * (size_t)nr));
  DV_TRY(w.label.ensure((size_t)nr));
  hipLaunchKernelGGL(fitgroups_count_kernel, dim3((unsigned)nr), dim3(MS_THREADS), 0, s, r0, nr, v.places, v.sfield, v.fptr, cs,
                     F, w.cnt.get());
  hipLaunchKernelGGL(fitgroups_scan_kernel, dim3(1), dim3(MS_THREADS), 0, s, nr, (const int*)w.cnt.get(), w.ptr.get());
  DV_HIP(hipGetLastError());
  int totals[2] = {0, 0};                              // the pairs (i, j <= i) and the adjacency entries
  DV_HIP(hipMemcpyAsync(&totals[0], w.ptr.get() + nr, sizeof(int), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(&totals[1], w.ptr.get() + 2 * (size_t)nr + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  const size_t npairs = (size_t)totals[0], nadj = (size_t)totals[1];
  if (totals[0] < 0 || totals[1] < 0 || nadj > 2 * npairs) {   // (more than 2^31 entries wrap the 32-bit scan)
    set_error("%s: fields %d .. %d: the overlapping pairs of %d galaxies do not fit 32-bit offsets", who, field_base + fa,
              field_base + fz, nr);
    return E_INVALID;
  }
  DV_TRY(w.pairs.ensure(std::max<size_t>(2 * npairs, 1)));
  DV_TRY(w.adj.ensure(std::max<size_t>(nadj, 1)));
  const int* adj_ptr = w.ptr.get() + nr + 1;
  hipLaunchKernelGGL(fitgroups_fill_kernel, dim3((unsigned)nr), dim3(MS_THREADS), 0, s, r0, nr, v.places, v.sfield, v.fptr, cs, F,
                     (const int*)w.ptr.get(), w.pairs.get(), w.adj.get());
  hipLaunchKernelGGL(fitgroups_label_kernel, dim3((unsigned)nf), dim3(MS_THREADS), 0, s, r0, nr, fa, v.fptr, adj_ptr,
                     (const int*)w.adj.get(), w.lab.get(), w.label.get());
  DV_HIP(hipGetLastError());
  w.label_h.resize((size_t)nr);
  DV_HIP(hipMemcpyAsync(w.label_h.data(), w.label.get(), (size_t)nr * sizeof(int), hipMemcpyDeviceToHost, s));
  if (lists) {
    lists->pairs.resize(2 * npairs);
    lists->adj_ptr.resize((size_t)nr + 1);
    lists->adj.resize(nadj);
    if (npairs) DV_HIP(hipMemcpyAsync(lists->pairs.data(), w.pairs.get(), 2 * npairs * sizeof(int), hipMemcpyDeviceToHost, s));
    DV_HIP(hipMemcpyAsync(lists->adj_ptr.data(), adj_ptr, ((size_t)nr + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    if (nadj) DV_HIP(hipMemcpyAsync(lists->adj.data(), w.adj.get(), nadj * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  DV_HIP(hipStreamSynchronize(s));

  // the grouping: a row whose label is its own row opens a group, and rows ascend, so the groups of a field come out ordered
  // by their smallest row and every group's members in ascending row order
  w.rtab_h.assign(2 * (size_t)nr, 0);
  w.gsize_h.assign((size_t)nr, 0);                     // by row of the launch: the group it opens, then that group's size
  w.gtab_h.clear();
  for (int f = fa; f <= fz; ++f) {
    const int a = fptr_h[f] - r0, z = fptr_h[f + 1] - r0;
    for (int i = a; i < z; ++i) {
      const int l = w.label_h[(size_t)i];
      if (l < 0 || l > i - a || w.label_h[(size_t)(a + l)] != l) {   // (cannot happen: a label is a root not above its row)
        set_error("%s: field %d: row %d came back with the label %d", who, field_base + f, i - a, l);
        return E_STATE;
      }
      if (l == i - a) {
        w.rtab_h[2 * (size_t)i] = (int)(w.gtab_h.size() / 4);
        w.gtab_h.insert(w.gtab_h.end(), {0, 0, 0, 0});
      }
      const int g = w.rtab_h[2 * (size_t)(a + l)];
      w.rtab_h[2 * (size_t)i] = g;
      w.rtab_h[2 * (size_t)i + 1] = (int)w.gtab_h[4 * (size_t)g + 2]++;
    }
    for (int i = a; i < z; ++i) {
      const long long n = w.gtab_h[4 * (size_t)w.rtab_h[2 * (size_t)i] + 2];
      group_h[(size_t)r0 + i] = w.label_h[(size_t)i];
      gsize_h[(size_t)r0 + i] = (int32_t)n;
      if (!v.stamps) continue;                       // (the groups alone: nothing is solved, nothing is refused)
      if (n > FF_MAX_N && w.label_h[(size_t)i] == i - a) {
        set_error("%s: field %d: the blend group of row %ld has %ld galaxies, the grouped fit takes at most %d per group", who,
                  field_base + f, (long)(i - a), (long)n, FF_MAX_N);
        return E_INVALID;
      }
      const size_t need = (size_t)nb * (size_t)n * (size_t)n * sizeof(double);
      if (need > (size_t)p.scratch_bytes && w.label_h[(size_t)i] == i - a) {
        set_error("%s: field %d: the blend group of row %ld has %ld galaxies: its Gram matrices need %zu bytes of scratch (bands x "
                  "n_g x n_g doubles), scratch_bytes is %ld", who, field_base + f, (long)(i - a), (long)n, need,
                  (long)p.scratch_bytes);
        return E_INVALID;
      }
    }
  }
  if (!v.stamps) {
    drain.dismiss();                                   // (the stream is idle behind the download of the labels)
    return OK;
  }
  // the slots, the scratch offsets and the sub-ranges
  const size_t ng = w.gtab_h.size() / 4, cap = (size_t)p.scratch_bytes / sizeof(double);
  std::vector<int> sub_first{0};                       // the first group of every sub-range
  size_t used = 0, most = 0;
  long long slot = 0;
  for (size_t g = 0; g < ng; ++g) {
    const size_t n = (size_t)w.gtab_h[4 * g + 2], need = (size_t)nb * n * n;
    if (used + need > cap) {
      sub_first.push_back((int)g);
      used = 0;
    }
    w.gtab_h[4 * g] = (long long)used;
    w.gtab_h[4 * g + 1] = slot;
    w.gtab_h[4 * g + 3] = (long long)sub_first.size() - 1;
    used += need;
    most = std::max(most, used);
    slot += (long long)n;
  }
  sub_first.push_back((int)ng);
  w.grows_h.resize((size_t)nr);
  for (int i = 0; i < nr; ++i) {
    const size_t g = (size_t)w.rtab_h[2 * (size_t)i];
    w.grows_h[(size_t)w.gtab_h[4 * g + 1] + (size_t)w.rtab_h[2 * (size_t)i + 1]] = r0 + i;
  }
  DV_TRY(w.rtab.ensure(2 * (size_t)nr));
  DV_TRY(w.grows.ensure((size_t)nr));
  DV_TRY(w.gtab.ensure(4 * ng));
  DV_TRY(w.scratch.ensure(std::max<size_t>(most, 1)));
  DV_HIP(hipMemcpyAsync(w.rtab, w.rtab_h.data(), 2 * (size_t)nr * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(w.grows, w.grows_h.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(w.gtab, w.gtab_h.data(), 4 * ng * sizeof(long long), hipMemcpyHostToDevice, s));
  // (a stamp wholly outside its field has no pair: its G_ii and h_i are the empty sums)
  DV_HIP(hipMemsetAsync(rows.gram + (size_t)r0 * nb, 0, (size_t)nr * nb * sizeof(double), s));
  DV_HIP(hipMemsetAsync(rows.proj + (size_t)r0 * nb, 0, (size_t)nr * nb * sizeof(double), s));
  for (size_t k = 0; k + 1 < sub_first.size(); ++k) {
    const int ga = sub_first[k], gz = sub_first[k + 1];
    if (gz <= ga) continue;
    const size_t last = (size_t)gz - 1, n = (size_t)w.gtab_h[4 * last + 2];
    const size_t elems = (size_t)w.gtab_h[4 * last] + (size_t)nb * n * n;
    DV_HIP(hipMemsetAsync(w.scratch, 0, elems * sizeof(double), s));
    if (npairs > 0) {
      fit_variant(v.weight != nullptr, 0, [&](auto wt, auto qc) {
        if constexpr (decltype(qc)::value == 0) {      // (the groups fit no sky)
          auto gram = [&](auto indexed) {              // (7y: the stamps through v.srow, in place on a resident set's store)
            hipLaunchKernelGGL((fitflux_gram_kernel<decltype(wt)::value, 0, true, decltype(indexed)::value>), dim3((unsigned)npairs),
                               dim3(MS_THREADS), 0, s, (const int*)w.pairs.get(), v.stamps, v.places, v.sfield, (const int*)nullptr,
                               (const long long*)nullptr, 0, v.f0, cs, nb, F, v.data, w.scratch.get(), rows.gram, rows.proj,
                               v.weight, (const int*)w.rtab.get(), (const long long*)w.gtab.get(), r0, (int)k, v.srow);
          };
          if (v.srow) gram(std::true_type{});
          else gram(std::false_type{});
        }
      });
    }
    hipLaunchKernelGGL((fitflux_solve_kernel<0, true>), dim3((unsigned)(gz - ga), (unsigned)nb), dim3(MS_THREADS), 0, s,
                       (const int*)nullptr, (const long long*)nullptr, ga, nb, p.min_pivot, w.scratch.get(),
                       (const double*)rows.gram, (const double*)rows.proj, rows.scale, rows.var, rows.status, (const double*)nullptr,
                       (double*)nullptr, (double*)nullptr, (int*)nullptr, (const int*)w.grows.get(), (const long long*)w.gtab.get());
    DV_HIP(hipGetLastError());
  }
  if (v.weight) {
    auto chi2 = [&](auto indexed) {
      hipLaunchKernelGGL((fitflux_chi2_kernel<0, decltype(indexed)::value>), dim3((unsigned)nr), dim3(MS_THREADS), 0, s, adj_ptr,
                         (const int*)w.adj.get(), r0, v.stamps, v.places, v.sfield, v.f0, cs, nb, F, v.data, v.weight,
                         (const double*)rows.scale, (const int*)rows.status, rows.chi2, rows.npix, (const double*)nullptr,
                         (const int*)nullptr, v.srow);
    };
    if (v.srow) chi2(std::true_type{});
    else chi2(std::false_type{});
    DV_HIP(hipGetLastError());
  }
  DV_HIP(hipStreamSynchronize(s));
  drain.dismiss();
  return OK;
}

// host arrays in, host rows out, whole fields at a time, as scene_fit_flux takes them: beside the scratch, the stamps, tables,
// rows and grouping tables of a run of fields
int scene_fit_flux_groups(const float* stamps_h, const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int nb,
                          const double* data_h, int M, int F, const FitFluxOut& rq, int device, hipStream_t s) {
  const char* who = rq.who;
  const bool weighted = rq.weights != nullptr;
  DV_TRY(fitflux_check(who, cs, nb, F, rq.par));
  if (N < 0 || M < 0 || !field_ptr || (N > 0 && (!data_h || !stamps_h || !places_h))) {
    set_error("%s: stamps, places, field_ptr and data_fields must all be given", who);
    return E_INVALID;
  }
  DV_TRY(fitflux_rows_check(who, rq.rows, N, weighted));
  if (!weighted && (rq.rows.chi2 || rq.rows.npix)) {
    set_error("%s: fit_chi2 and fit_npix are the outputs of the weighted fit: without weight_fields both must be NULL", who);
    return E_INVALID;
  }
  if (N > 0 && (!rq.group || !rq.group_size)) {
    set_error("%s: fit_group and fit_group_size must all be given", who);
    return E_INVALID;
  }
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, nullptr, nullptr));
  if (N == 0) return OK;
  FieldStamps v{};
  v.cs = cs, v.nb = nb, v.F = F;
  FitFluxRows d{};
  Rows in, out;
  in.add(v.stamps, stamps_h, (size_t)cs * cs * nb);
  in.add(v.places, places_h, 2);
  fitflux_columns(out, d, rq.rows, nb, weighted, false);
  WholeFields f{nullptr, data_h, rq.weights, FitGroupsWork::BYTES_PER_ROW, 0, (size_t)rq.par.scratch_bytes, false};
  DV_HIP(hipSetDevice(device));
  FitGroupsWork work;
  return walk_whole_fields(who, M, field_ptr, N, f, v, in, out, s, [&](const FieldStamps& run, int fa, int nf, int64_t r0,
                                                                         const int* fptr_h) {
    return launch_fit_flux_groups(who, run, fptr_h, 0, nf - 1, fa, rq.par, work, d, rq.group + r0, rq.group_size + r0, nullptr, s);
  });
}

namespace {
// the refusals of a resident set's call for its outputs: every output the chosen variant produces, and no other
int field_set_outputs_check(const char* who, const FitFluxOut& rq, int64_t N) {
  const FitFluxRows& o = rq.rows;
  const FitFluxSky& sky = rq.sky;
  const FitFluxNonneg& nn = rq.nonneg;
  if (nn.on && nn.max_iter < 1) {
    set_error("%s: max_iter must be at least 1 (got %d)", who, nn.max_iter);
    return E_INVALID;
  }
  if (N > 0 && (!o.scale || !o.var || !o.gram || !o.proj || !o.status)) {
    set_error("%s: fit_scale, fit_var, fit_gram, fit_proj and fit_status must all be given", who);
    return E_INVALID;
  }
  if (rq.weights ? (N > 0 && (!o.chi2 || !o.npix)) : (o.chi2 || o.npix)) {
    set_error("%s: fit_chi2 and fit_npix are the outputs of the weighted fit: both given with weight, both NULL without", who);
    return E_INVALID;
  }
  if (rq.sky_order >= 0 ? (!sky.coef || !sky.cov || !sky.status || !sky.npix) : (sky.coef || sky.cov || sky.status || sky.npix)) {
    set_error("%s: sky_coef, sky_cov, sky_status and sky_npix are the outputs of the fit with sky: all given with sky_order 0 or "
              "1, all NULL with -1", who);
    return E_INVALID;
  }
  if (nn.on ? (!nn.iters || !nn.status || (N > 0 && (!o.scale_free || !o.clamped || !o.dual)))
            : (o.scale_free || o.clamped || o.dual || nn.iters || nn.status)) {
    set_error("%s: fit_scale_free, fit_clamped, fit_dual, nonneg_iters and nonneg_status are the outputs of the non-negative fit: "
              "all given with nonneg, all NULL without", who);
    return E_INVALID;
  }
  if (rq.grouped() && N > 0 && (!rq.group || !rq.group_size)) {
    set_error("%s: fit_group and fit_group_size must all be given", who);
    return E_INVALID;
  }
  return OK;
}
}  // namespace

// The rows go through the kernels in joint order (joint_order, rows.h) and leave in resident-row order: they are downloaded into
// host staging and scattered through rowmap.  Dense: the stamps, placements and fields are regrouped into a copy on the device
// and launch_fit_flux runs on the copy.  Grouped: only the per-row scalars - placement, field and srow = rowmap - are uploaded in
// joint order, and launch_fit_flux_groups reads the stamps in place through srow.
int field_set_fit_flux(const ResidentRows& set, const double* data_h, const FitFluxOut& rq, int device, hipStream_t s) {
  const char* who = rq.who;
  const int M = set.M, F = set.F, nb = set.nb, cs = set.cs;
  const int64_t N = (int64_t)set.nrows;
  const bool weighted = rq.weights != nullptr, grouped = rq.grouped();
  DV_TRY(fitflux_check(who, cs, nb, F, rq.par));
  DV_TRY(field_set_outputs_check(who, rq, N));
  if (!data_h && !set.base) {
    set_error("%s: a cumulative set keeps no copy of the fields as uploaded (every pass subtracts from the working residual): "
              "data must be given", who);
    return E_INVALID;
  }
  const JointOrder jo = joint_order(set.pass_fptr, M);
  if (jo.fptr64[(size_t)M] != N) {                      // (cannot happen: both count the passes that kept rows)
    set_error("%s: the passes on record hold %ld rows, the set %zu", who, (long)jo.fptr64[(size_t)M], set.nrows);
    return E_STATE;
  }
  FitFluxPlan plan;
  if (!grouped) DV_TRY(fitflux_plan(who, jo.fptr64.data(), M, nb, rq.par, &plan, rq.sky_order, F));
  if (N == 0) return OK;
  const std::vector<int32_t> places_h = jo.places(set.places_h);
  const int q = plan.q;
  const size_t stamp = (size_t)cs * cs * nb, felems = (size_t)F * F * nb;
  FitFluxRows d{};
  Rows out;
  fitflux_columns(out, d, rq.rows, nb, weighted, rq.nonneg.on);
  RowStage stage;
  stage.take(out, N);
  int32_t* const group_j = grouped ? (int32_t*)stage.add(rq.group, sizeof(int32_t), N) : nullptr;
  int32_t* const gsize_j = grouped ? (int32_t*)stage.add(rq.group_size, sizeof(int32_t), N) : nullptr;
  DV_HIP(hipSetDevice(device));
  // what the call holds beside the set: the tables in joint order, the rows, the fields it uploads, and - dense - the regrouped
  // copy, the dense scratch and the per-field outputs, or - grouped - the group tables and lists (the lists at the two entries
  // per row the stand-alone call counts; their true size is known behind the count kernel and allocated there) and the scratch:
  // at most scratch_bytes, and never more than every field dense, which no sub-range exceeds.  No second copy of the stamps.
  const size_t fields_b = ((data_h ? 1 : 0) + (weighted ? 1 : 0)) * (size_t)M * felems * sizeof(double);
  size_t need = 0;
  if (grouped) {
    size_t dense = 0;                                   // sum nb n_f^2
    for (int f = 0; f < M; ++f) {
      const size_t n = (size_t)(jo.fptr64[(size_t)f + 1] - jo.fptr64[(size_t)f]);
      dense += (size_t)nb * n * n;
    }
    const size_t scratch_b = std::min((size_t)rq.par.scratch_bytes, dense * sizeof(double));
    need = (size_t)N * (4 * sizeof(int) + FitGroupsWork::BYTES_PER_ROW + out.bytes()) + ((size_t)M + 1) * sizeof(int) + scratch_b +
           fields_b;
  } else {
    need = (size_t)N * (stamp * sizeof(float) + 4 * sizeof(int) + out.bytes()) + ((size_t)M + 1) * sizeof(int) +
           FitFluxWork::bytes(plan, (size_t)M, weighted) + FitFluxFieldOut::bytes(q, rq.nonneg.on, (size_t)M, nb) + fields_b;
  }
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b / 10 * 9) {
    if (grouped)
      set_error("%s: the tables of %ld rows, the scratch of the groups and the uploaded fields need %zu bytes of device memory, %zu "
                "are free", who, (long)N, need, free_b);
    else
      set_error("%s: the regrouped stamps of %ld rows, the dense scratch and the uploaded fields need %zu bytes of device memory, "
                "%zu are free", who, (long)N, need, free_b);
    return E_NOMEM;
  }
  DevBuf<float> stamps;
  DevBuf<int> places, sf, rmap, fptr;
  const double* const field_h[2] = {data_h, rq.weights};
  DevBuf<double> field_d[2];
  FitFluxWork work;
  FitFluxFieldOut fout;
  FitGroupsWork gwork;
  if (!grouped) DV_TRY(stamps.alloc((size_t)N * stamp));
  DV_TRY(places.alloc((size_t)N * 2));
  DV_TRY(sf.alloc((size_t)N));
  DV_TRY(rmap.alloc((size_t)N));
  DV_TRY(fptr.alloc((size_t)M + 1));
  if (!grouped) DV_TRY(work.alloc(plan, M, weighted));
  DV_TRY(out.alloc(N));
  if (!grouped) DV_TRY(fout.alloc(q, rq.nonneg, (size_t)M, nb));
  StreamDrain drain(s);                                // a failure waits for the stream before the call's buffers go
  for (int k = 0; k < 2; ++k)
    if (field_h[k]) {
      DV_TRY(field_d[k].alloc((size_t)M * felems));
      DV_HIP(hipMemcpyAsync(field_d[k], field_h[k], (size_t)M * felems * sizeof(double), hipMemcpyHostToDevice, s));
    }
  FieldStamps v{set.stamps, places, sf, fptr, data_h ? field_d[0].get() : set.base, field_d[1].get(), nullptr, 0, cs, nb, F};
  if (grouped) {
    DV_HIP(hipMemcpyAsync(places, places_h.data(), (size_t)N * 2 * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(sf, jo.sfield.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
  }
  DV_HIP(hipMemcpyAsync(rmap, jo.rowmap.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(fptr, jo.fptr32.data(), ((size_t)M + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  if (grouped) {
    v.srow = rmap;
    DV_TRY(launch_fit_flux_groups(who, v, jo.fptr32.data(), 0, M - 1, 0, rq.par, gwork, d, group_j, gsize_j, nullptr, s));
    DV_TRY(out.download(0, N, s));
  } else {
    DV_TRY(launch_fitflux_regroup(rmap, set.stamps, set.places, set.field, N, cs, nb, stamps, places, sf, s));
    v.stamps = stamps;
    DV_TRY(launch_fit_flux(v, places_h.data(), jo.fptr32.data(), 0, M - 1, rq.par, work, d, fout.sky, fout.nonneg, true, s));
    DV_TRY(out.download(0, N, s));
    DV_TRY(fout.download(rq.sky, rq.nonneg, 0, 0, (size_t)M, nb, s));
  }
  DV_HIP(hipStreamSynchronize(s));
  drain.dismiss();
  stage.scatter(jo.rowmap.data(), N);                  // joint row k is resident row rowmap[k]
  return OK;
}


// the blend groups alone, from the placements: no stamps, no fit, no limit on a group.  n_pairs / n_adj are always written;
// pairs [n_pairs][2], adj_ptr [N + 1] and adj [n_adj] - the lists the fit works from, rows of the call - where they are given
int scene_fit_groups(const int32_t* places_h, const int64_t* field_ptr, int64_t N, int cs, int M, int F, int32_t* group_h,
                     int32_t* gsize_h, int64_t pair_cap, int64_t* n_pairs, int32_t* pairs_h, int64_t adj_cap, int64_t* n_adj,
                     int32_t* adj_ptr_h, int32_t* adj_h, int device, hipStream_t s) {
  const char* who = "dv_scene_fit_groups";
  DV_TRY(fitflux_check(who, cs, 1, F, FitFluxParams{0.5, 1}));
  if (N < 0 || M < 0 || !field_ptr || !n_pairs || !n_adj || (N > 0 && (!places_h || !group_h || !gsize_h))) {
    set_error("%s: places, field_ptr, fit_group, fit_group_size, n_pairs and n_adj must all be given", who);
    return E_INVALID;
  }
  if ((pairs_h == nullptr) != (adj_h == nullptr) || (pairs_h == nullptr) != (adj_ptr_h == nullptr)) {
    set_error("%s: pairs, adj_ptr and adj go together (all given or all NULL)", who);
    return E_INVALID;
  }
  std::vector<int32_t> sf_h;
  std::vector<int> fptr_h;
  DV_TRY(field_tables(who, "stamps", M, field_ptr, N, &F, places_h, &sf_h, &fptr_h));
  *n_pairs = *n_adj = 0;
  if (adj_ptr_h) std::fill(adj_ptr_h, adj_ptr_h + N + 1, 0);
  if (N == 0) return OK;
  DV_HIP(hipSetDevice(device));
  DevBuf<int> places, sf, fptr;
  DV_TRY(places.alloc((size_t)N * 2));
  DV_TRY(sf.alloc((size_t)N));
  DV_TRY(fptr.alloc((size_t)M + 1));
  FitGroupsWork work;
  FitGroupsLists lists;
  StreamDrain drain(s);
  DV_HIP(hipMemcpyAsync(places, places_h, (size_t)N * 2 * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(sf, sf_h.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(fptr, fptr_h.data(), ((size_t)M + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  const FieldStamps v{nullptr, places, sf, fptr, nullptr, nullptr, nullptr, 0, cs, 1, F};
  DV_TRY(launch_fit_flux_groups(who, v, fptr_h.data(), 0, M - 1, 0, FitFluxParams{0.5, 1}, work, FitFluxRows{}, group_h, gsize_h,
                                &lists, s));
  drain.dismiss();
  *n_pairs = (int64_t)(lists.pairs.size() / 2);
  *n_adj = (int64_t)lists.adj.size();
  if (pairs_h) {
    if (*n_pairs > pair_cap || *n_adj > adj_cap) {
      set_error("%s: %ld pairs and %ld adjacency entries, the arrays given hold %ld and %ld", who, (long)*n_pairs, (long)*n_adj,
                (long)pair_cap, (long)adj_cap);
      return E_INVALID;
    }
    std::copy(lists.pairs.begin(), lists.pairs.end(), pairs_h);
    std::copy(lists.adj_ptr.begin(), lists.adj_ptr.end(), adj_ptr_h);
    std::copy(lists.adj.begin(), lists.adj.end(), adj_h);
  }
  return OK;
}

// step 1 of one field alone: host arrays in, G [nb][n][n] (the lower triangle, zeros above) and h [n][nb] out
int scene_fit_flux_gram(const float* stamps_h, const int32_t* places_h, int64_t n, int cs, int nb, const double* data_h, int F,
                        double* gram_h, double* proj_h, int device, hipStream_t s) {
  const char* who = "dv_scene_fit_flux_gram";
  if (n > FF_MAX_N) {
    set_error("%s: field 0 has %ld galaxies, the dense fit takes at most %d per field", who, (long)n, FF_MAX_N);
    return E_INVALID;
  }
  const size_t need = (size_t)nb * (size_t)std::max<int64_t>(n, 0) * (size_t)std::max<int64_t>(n, 0) * sizeof(double);
  const FitFluxParams p{0.5, (int64_t)std::max<size_t>(need, 1)};
  DV_TRY(fitflux_check(who, cs, nb, F, p));
  if (n < 0 || (n > 0 && (!stamps_h || !places_h || !data_h || !gram_h || !proj_h))) {
    set_error("%s: stamps, places, data_field, gram and proj must all be given", who);
    return E_INVALID;
  }
  for (int64_t i = 0; i < n; ++i) DV_TRY(place_check(who, i, places_h));
  const int64_t field_ptr[2] = {0, n};
  FitFluxPlan plan;
  DV_TRY(fitflux_plan(who, field_ptr, 1, nb, p, &plan, -1, F));
  if (n == 0) return OK;
  const size_t stamp = (size_t)cs * cs * nb, felems = (size_t)F * F * nb;
  DV_HIP(hipSetDevice(device));
  DevBuf<float> stamps;
  DevBuf<double> data, gram, proj;
  DevBuf<int> places, sf, fptr;
  FitFluxWork work;
  DV_TRY(work.alloc(plan, 1, false));   // (step 1 alone: no adjacency)
  DV_TRY(stamps.alloc((size_t)n * stamp));
  DV_TRY(places.alloc((size_t)n * 2));
  DV_TRY(sf.alloc((size_t)n));
  DV_TRY(fptr.alloc(2));
  DV_TRY(data.alloc(felems));
  DV_TRY(gram.alloc((size_t)n * nb));
  DV_TRY(proj.alloc((size_t)n * nb));
  const int fptr_h[2] = {0, (int)n};
  StreamDrain drain(s);
  DV_HIP(hipMemcpyAsync(stamps, stamps_h, (size_t)n * stamp * sizeof(float), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(places, places_h, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemsetAsync(sf, 0, (size_t)n * sizeof(int), s));
  DV_HIP(hipMemcpyAsync(fptr, fptr_h, sizeof(fptr_h), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(data, data_h, felems * sizeof(double), hipMemcpyHostToDevice, s));
  const FitFluxRows rows{nullptr, nullptr, gram.get(), proj.get(), nullptr};
  const FieldStamps v{stamps, places, sf, fptr, data, nullptr, nullptr, 0, cs, nb, F};
  DV_TRY(launch_fit_flux(v, places_h, fptr_h, 0, 0, p, work, rows, FitFluxSky{}, FitFluxNonneg{}, false, s));
  DV_HIP(hipMemcpyAsync(gram_h, work.scratch, need, hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(proj_h, proj, (size_t)n * nb * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  drain.dismiss();
  return OK;
}

// step 1 of the bordered system of one field (7t): host arrays in; G, E and K [nb][n + q][n + q] (the lower triangle, zeros
// above) and the right-hand side h, c [n + q][nb] out - the bits the solve of dv_scene_fit_flux_sky starts from
int scene_fit_flux_sky_gram(const float* stamps_h, const int32_t* places_h, int64_t n, int cs, int nb, const double* data_h,
                            const double* weight_h, int F, int sky_order, double* gram_h, double* rhs_h, int device, hipStream_t s) {
  const char* who = "dv_scene_fit_flux_sky_gram";
  if (sky_order != 0 && sky_order != 1) {
    set_error("%s: sky_order must be 0 (a constant) or 1 (a plane), got %d", who, sky_order);
    return E_INVALID;
  }
  if (n > FF_MAX_N) {
    set_error("%s: field 0 has %ld galaxies, the dense fit takes at most %d per field", who, (long)n, FF_MAX_N);
    return E_INVALID;
  }
  const int q = fitflux_sky_q(sky_order);
  const size_t nt = (size_t)std::max<int64_t>(n, 0) + q;
  const size_t need = (size_t)nb * nt * nt * sizeof(double);
  const FitFluxParams p{0.5, (int64_t)need};
  DV_TRY(fitflux_check(who, cs, nb, F, p));
  if (n < 0 || !data_h || !gram_h || !rhs_h || (n > 0 && (!stamps_h || !places_h))) {
    set_error("%s: stamps, places, data_field, gram and rhs must all be given", who);
    return E_INVALID;
  }
  for (int64_t i = 0; i < n; ++i) DV_TRY(place_check(who, i, places_h));
  const int64_t field_ptr[2] = {0, n};
  FitFluxPlan plan;
  DV_TRY(fitflux_plan(who, field_ptr, 1, nb, p, &plan, sky_order, F));
  const size_t stamp = (size_t)cs * cs * nb, felems = (size_t)F * F * nb, acc = fitflux_sky_acc(q);
  DV_HIP(hipSetDevice(device));
  DevBuf<float> stamps;
  DevBuf<double> data, wdata, gram, proj, coef, cov;
  DevBuf<int> places, sf, fptr, status;
  DevBuf<long long> npix;
  FitFluxWork work;
  DV_TRY(work.alloc(plan, 1, false));   // (step 1 alone: no adjacency)
  DV_TRY(stamps.alloc((size_t)n * stamp));
  DV_TRY(places.alloc((size_t)n * 2));
  DV_TRY(sf.alloc((size_t)n));
  DV_TRY(fptr.alloc(2));
  DV_TRY(data.alloc(felems));
  if (weight_h) DV_TRY(wdata.alloc(felems));
  DV_TRY(gram.alloc((size_t)n * nb));
  DV_TRY(proj.alloc((size_t)n * nb));
  DV_TRY(npix.alloc((size_t)nb));
  const int fptr_h[2] = {0, (int)n};
  StreamDrain drain(s);
  if (n > 0) {
    DV_HIP(hipMemcpyAsync(stamps, stamps_h, (size_t)n * stamp * sizeof(float), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(places, places_h, (size_t)n * 2 * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemsetAsync(sf, 0, (size_t)n * sizeof(int), s));
  }
  DV_HIP(hipMemcpyAsync(fptr, fptr_h, sizeof(fptr_h), hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(data, data_h, felems * sizeof(double), hipMemcpyHostToDevice, s));
  if (weight_h) DV_HIP(hipMemcpyAsync(wdata, weight_h, felems * sizeof(double), hipMemcpyHostToDevice, s));
  const FitFluxRows rows{nullptr, nullptr, gram.get(), proj.get(), nullptr};
  const FitFluxSky sky{q, nullptr, nullptr, nullptr, npix.get()};
  const FieldStamps v{stamps, places, sf, fptr, data, weight_h ? wdata.get() : nullptr, nullptr, 0, cs, nb, F};
  DV_TRY(launch_fit_flux(v, places_h, fptr_h, 0, 0, p, work, rows, sky, FitFluxNonneg{}, false, s));
  std::vector<double> sums((size_t)nb * acc);
  DV_HIP(hipMemcpyAsync(gram_h, work.scratch, need, hipMemcpyDeviceToHost, s));
  if (n > 0) DV_HIP(hipMemcpyAsync(rhs_h, proj, (size_t)n * nb * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipMemcpyAsync(sums.data(), work.sky_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  drain.dismiss();
  for (int b = 0; b < nb; ++b)
    for (int t = 0; t < q; ++t) rhs_h[((size_t)n + t) * nb + b] = sums[(size_t)b * acc + (size_t)q * (q + 1) / 2 + t];
  return OK;
}

}  // namespace dv
