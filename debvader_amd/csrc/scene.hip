// Scene compositing around the network: cutout gather and the residual / predicted fields.
//
// Reference behaviour restated:
//  * extract/extraction.py:4-43       cutout i = field[0, xs:xs+cs, ys:ys+cs, :] (callers validate the window)
//  * deblend/field_deblender.py:46-97   residual  = field - sum_i shift(pad(mean_i), (x_i, y_i))        (in object order)
//  * deblend/field_deblender.py:99-189  predicted = sum_i shift(pad(stamp_i), (x_i, y_i)) for mean / stddev / epistemic
//    where pad() centres the cs x cs stamp in a zero F x F image and shift() is scipy.ndimage.shift with its defaults
//    (cubic B-spline, mode "constant", prefilter on).  The reference builds an F x F image per object and band and
//    shifts it on the CPU (its own TODO at :82 calls this "super slow").
//
// Here: float64 like the reference's numpy arrays; one thread per field element walks the objects IN ORDER (same
// summation order as the reference loop, so results are deterministic and agree to rounding).  An object whose two
// shifts are integers is an exact translation (no spline needed: interpolating a spline at its knots returns the
// samples).  Other objects get cubic B-spline coefficients of the zero-extended stamp (recursive prefilter, pole
// sqrt(3)-2, margin T = 20 pixels: 0.268^20 = 4e-12) and are evaluated with the 4 x 4 B-spline weights.
// HBM-bound byte work; nothing here wants MFMA.
#include "common.h"

namespace dv {

namespace {
constexpr int T_MARGIN = 20;

struct SceneObj {
  double sx, sy;     // shift of the stamp's top-left corner relative to field index 0 (po + pos), rows / cols
  int ix, iy;        // the same as integers (integer objects)
  int coef;          // index into the coefficient buffer, -1 for integer objects
  int pad_;
};

// Cutout gather (extract/extraction.py:4-43), one workgroup per cutout; a wave copies every fourth row, 64 consecutive
// elements (pixel-major, band-minor) per trip: coalesced on both sides and no index arithmetic beyond one multiply per row
// (the first version decoded a flat 64-bit element index with four divisions per element: 1.08 ms per 8192-cutout chunk of
// the inference pipeline, 0.41 ms now).  OUT = double: the reference's cutouts; OUT = float: cast as deblend() does
// (tf.cast, deblender.py:18), straight into the network's input buffer.
// `field` is the first resident field f0 of a stack of F x F x nb fields and sfield[n] the field cutout n is cut from - one
// lookup per workgroup, uniform for all its threads.  sfield = null (dv_scene_extract only): one field.
template <typename OUT>
__global__ __launch_bounds__(256) void scene_extract_kernel(const double* __restrict__ field, int F, int nb,
                                                            const int* __restrict__ starts, int cs, OUT* __restrict__ out,
                                                            const int* __restrict__ sfield, int f0) {
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = starts[2 * n], y0 = starts[2 * n + 1];
  if (sfield) field += (long)(sfield[n] - f0) * F * F * nb;
  const int rowlen = cs * nb;
  OUT* o = out + (long)n * cs * rowlen;
  for (int i = wave; i < cs; i += 4) {
    const double* src = field + ((long)(x0 + i) * F + y0) * nb;
    OUT* dst = o + (long)i * rowlen;
    for (int x = lane; x < rowlen; x += 64) dst[x] = (OUT)src[x];
  }
}

// cubic B-spline coefficients of one stamp plane set st [cs][cs][nb] (float64, or the network's float32 cast exactly)
// zero-extended by T on every side: c [P][P][nb].  One workgroup.
template <typename T>
__device__ __forceinline__ void scene_prefilter_body(const T* __restrict__ st, int cs, int nb, double* __restrict__ c) {
  const int P = cs + 2 * T_MARGIN;
  const double z1 = -0.26794919243112270647;   // sqrt(3) - 2
  // axis 0 (rows) for the cs stamp columns; the other columns of the extended image are zero and stay zero
  for (int t = threadIdx.x; t < cs * nb; t += 256) {
    const int j = t / nb, b = t - j * nb;
    double* col = c + ((long)(T_MARGIN + j)) * nb + b;          // element [k][T+j][b] at col[k * P * nb]
    const long ks = (long)P * nb;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
      const int i = k - T_MARGIN;
      const double s = (i >= 0 && i < cs) ? (double)st[((long)i * cs + j) * nb + b] : 0.0;
      acc = 6.0 * s + z1 * acc;
      col[k * ks] = acc;
    }
    double nxt = 0.0;
    for (int k = P - 1; k >= 0; --k) {
      nxt = z1 * (nxt - col[k * ks]);
      col[k * ks] = nxt;
    }
  }
  __syncthreads();
  // axis 1 (columns) for every row
  for (int t = threadIdx.x; t < P * nb; t += 256) {
    const int k = t / nb, b = t - k * nb;
    double* row = c + (long)k * P * nb + b;                       // element [k][j][b] at row[j * nb]
    double acc = 0.0;
    for (int j = 0; j < P; ++j) {
      const int jj = j - T_MARGIN;
      const double s = (jj >= 0 && jj < cs) ? row[(long)j * nb] : 0.0;
      acc = 6.0 * s + z1 * acc;
      row[(long)j * nb] = acc;
    }
    double nxt = 0.0;
    for (int j = P - 1; j >= 0; --j) {
      nxt = z1 * (nxt - row[(long)j * nb]);
      row[(long)j * nb] = nxt;
    }
  }
}

// coefficients of stamp which[k] of the chunk: coef[k][P][P][nb]
__global__ __launch_bounds__(256) void scene_prefilter_kernel(const double* __restrict__ stamps,
                                                              const int* __restrict__ which, int cs, int nb,
                                                              double* __restrict__ coef) {
  const int P = cs + 2 * T_MARGIN;
  scene_prefilter_body(stamps + (long)which[blockIdx.x] * cs * cs * nb, cs, nb, coef + (long)blockIdx.x * P * P * nb);
}

__device__ __forceinline__ void bspline3(double t, double w[4]) {
  const double u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
  w[2] = (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0;
  w[3] = t * t * t / 6.0;
}

// shift(pad(stamp), pos) at field pixel (r, c) from the stamp's coefficients, for NP planes of NB consecutive bands each
// (cf[p] = band 0 of plane p's [P][P][nb] coefficients); false: the pixel gets nothing from this object.
// scipy.ndimage.shift, mode "constant": output is cval where the input coordinate leaves [0, F-1]; the spline
// coefficients are those of the F x F padded image with MIRROR boundaries at its edge samples, and nodes
// outside the image are looked up mirrored.  With the infinite-domain coefficients cinf of the zero-extended
// stamp (what the prefilter computes) the mirrored ones are cm[i] = cinf[i] + cinf[-i] + cinf[2(F-1)-i].
// The reflected terms vanish unless the padded stamp sits within ~T pixels of the image edge (po < T).
// The 4 x 4 weights and the tap indices are worked out once for all planes and bands.
template <int NP, int NB>
__device__ __forceinline__ bool scene_spline_eval(const double* const (&cf)[NP], int nbands, int nb, int cs, int F, int po,
                                                  double sx, double sy, int r, int c, double (&v)[NP][NB]) {
  const int P = cs + 2 * T_MARGIN;
  const double xin = (double)r - (sx - po), yin = (double)c - (sy - po);
  if (xin < 0.0 || yin < 0.0 || xin > F - 1.0 || yin > F - 1.0) return false;
  const int off = po - T_MARGIN;                 // padded-image index of coefficient-image index 0
  const bool refl = off < 2;
  if (!refl && (xin - off < -2.0 || yin - off < -2.0 || xin - off > P + 1.0 || yin - off > P + 1.0)) return false;
  const double fx = floor(xin), fy = floor(yin);
  double wx[4], wy[4];
  bspline3(xin - fx, wx);
  bspline3(yin - fy, wy);
  const int nr = refl ? 3 : 1;
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int b = 0; b < NB; ++b) v[p][b] = 0.0;
  for (int a = 0; a < 4; ++a) {
    int i = (int)fx - 1 + a;
    i = i < 0 ? -i : (i > F - 1 ? 2 * (F - 1) - i : i);
    const int ri[3] = {i - off, -i - off, 2 * (F - 1) - i - off};
    for (int d = 0; d < 4; ++d) {
      int j = (int)fy - 1 + d;
      j = j < 0 ? -j : (j > F - 1 ? 2 * (F - 1) - j : j);
      const int rj[3] = {j - off, -j - off, 2 * (F - 1) - j - off};
      double cm[NP][NB];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int b = 0; b < NB; ++b) cm[p][b] = 0.0;
      for (int u = 0; u < nr; ++u) {
        if ((unsigned)ri[u] >= (unsigned)P) continue;
        for (int w = 0; w < nr; ++w)
          if ((unsigned)rj[w] < (unsigned)P) {
            const long ce = ((long)ri[u] * P + rj[w]) * nb;
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
              for (int b = 0; b < NB; ++b)
                if (b < nbands) cm[p][b] += cf[p][ce + b];
          }
      }
      const double wgt = wx[a] * wy[d];
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int b = 0; b < NB; ++b) v[p][b] += wgt * cm[p][b];
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void scene_composite_kernel(double* __restrict__ field, int F, int nb,
                                                              const double* __restrict__ stamps,
                                                              const double* __restrict__ coef,
                                                              const SceneObj* __restrict__ objs, int nobj, int cs,
                                                              int po, double sign) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)F * F * nb) return;
  const int b = (int)(e % nb);
  const long px = e / nb;
  const int c = (int)(px % F), r = (int)(px / F);
  const int P = cs + 2 * T_MARGIN;
  double acc = field[e];
  for (int o = 0; o < nobj; ++o) {
    const SceneObj ob = objs[o];
    if (ob.coef < 0) {
      const int rr = r - ob.ix, cc = c - ob.iy;
      if ((unsigned)rr < (unsigned)cs && (unsigned)cc < (unsigned)cs)
        acc += sign * stamps[(((long)o * cs + rr) * cs + cc) * nb + b];
      continue;
    }
    const double* const cf[1] = {coef + (long)ob.coef * P * P * nb + b};
    double v[1][1];
    if (scene_spline_eval<1, 1>(cf, 1, nb, cs, F, po, ob.sx, ob.sy, r, c, v)) acc += sign * v[0][0];
  }
  field[e] = acc;
}

// ---- compositing of one inference chunk, device resident (dv_infer_cutouts_composite) --------------------------------
// field += stamp_i placed with its top-left corner at places[i] = (row, col), for the n stamps of a chunk IN OBJECT ORDER
// per field element - the order of the reference's loop over res_deblend (field_deblender.py:112-183: one
// scipy.ndimage.shift of a padded image per object, integer shifts) and of scene_composite_kernel above, so the sums are
// bit-identical to the host-composited path.  Stamps are the network's float32 outputs as the forward pass left them in
// HBM (mean and stddev of every stamp, 167 KB per stamp that never cross the host link).
//
// A workgroup owns a 32 x 32-pixel tile of the field (four pixels per thread) and scans the chunk's objects in rounds of 2048 (eight per thread,
// their placements by four 16-byte loads): the objects whose window meets the tile are compacted IN ORDER into an LDS
// list (a prefix sum of the hit counts over the 256 threads), then every thread walks the list for its pixel.  Uniformly
// scattered cutouts leave ~4 entries per round and tile; a pile of objects on one spot just makes the lists long (a
// round's list holds all 2048) - no capacity limit, no atomics, no float non-determinism.
//
// The three result pointers address a stack of fields starting at field f0 (one field for dv_infer_cutouts_composite),
// blockIdx.y + fy0 is the field this workgroup's tile belongs to, and the workgroup scans only that field's objects
// of the chunk: fptr[m] .. fptr[m + 1] (global stamp numbers) cut to the chunk [obase, obase + n).  A field has its own
// workgroups, so two fields never meet in a sum, and within a field the order of additions is object order: a field's
// result has the same bits whatever other fields the call holds.  A field without objects in the chunk returns at once.
//
// X4, a fourth sum with the placement, the object order and the load-add-store across chunks of the other three (the
// instantiation without it is the kernel as it was):
//  X4_EPS  (dv_infer_fields_mc_composite): eps_f += the chunk's Monte-Carlo std stamps `eps` (float32, one per stamp, as the
//          Welford fold left them);
//  X4_RES2 (dv_field_set_pass, reference mode): eps_f -= the mean stamps, a second residual beside res_f - the pass's
//          working residual starts from the base field, the set's `final` continues the earlier passes.
constexpr int CT = 32;       // tile edge: a thread owns the four pixels (ty + 16 a, tx + 16 b) of its 32 x 32 tile
constexpr int CSEG = 2048;   // objects per scan round (8 per thread)
constexpr int X4_NONE = 0, X4_EPS = 1, X4_RES2 = 2;
template <int NBMAX, int X4>
__global__ __launch_bounds__(256) void scene_composite_chunk_kernel(double* __restrict__ mean_f, double* __restrict__ std_f,
                                                                    double* __restrict__ res_f, int F, int nb,
                                                                    const float* __restrict__ loc,
                                                                    const float* __restrict__ scale,
                                                                    const int* __restrict__ places, int n, int cs,
                                                                    const int* __restrict__ fptr, int f0, int fy0,
                                                                    long obase, double* __restrict__ eps_f,
                                                                    const float* __restrict__ eps) {
  __shared__ int s_list[CSEG];        // objects of the round that meet the tile, in object order
  __shared__ int s_lr[CSEG], s_lc[CSEG];   // their placements
  __shared__ int s_wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntx = (F + CT - 1) / CT;
  const int tr0 = (blockIdx.x / ntx) * CT, tc0 = (blockIdx.x % ntx) * CT;
  const int ty = tid >> 4, tx = tid & 15;
  constexpr bool EPS = X4 != X4_NONE;
  double am[4][NBMAX], as[4][NBMAX], ar[4][NBMAX], ae[EPS ? 4 : 1][NBMAX];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int b = 0; b < NBMAX; ++b) {
      am[q][b] = as[q][b] = ar[q][b] = 0.0;
      if constexpr (EPS) ae[q][b] = 0.0;
    }
  bool loaded = false;
  unsigned touched = 0;
  const int m = fy0 + (int)blockIdx.y;   // uniform over the workgroup
  const long lo = (long)fptr[m] - obase, hi = (long)fptr[m + 1] - obase;
  const int olo = (int)(lo > 0 ? lo : 0);
  n = (int)(hi < n ? hi : n);
  if (olo >= n) return;
  const long fo = (long)(m - f0) * F * F * nb;
  mean_f += fo;
  std_f += fo;
  if (res_f) res_f += fo;
  if constexpr (EPS) eps_f += fo;
  for (int seg = olo; seg < n; seg += CSEG) {
    // thread t tests objects seg + 8 t .. + 7 (four 16-byte loads of their placements): order by (thread, bit) = object order
    const int o0 = seg + tid * 8;
    unsigned hits = 0;
    int pr[8], pc[8];
    if (o0 + 8 <= n && (reinterpret_cast<size_t>(places + 2 * o0) & 15) == 0) {
      const int4* q = reinterpret_cast<const int4*>(places + 2 * o0);
      const int4 a = q[0], b = q[1], d = q[2], e = q[3];
      pr[0] = a.x; pc[0] = a.y; pr[1] = a.z; pc[1] = a.w; pr[2] = b.x; pc[2] = b.y; pr[3] = b.z; pc[3] = b.w;
      pr[4] = d.x; pc[4] = d.y; pr[5] = d.z; pc[5] = d.w; pr[6] = e.x; pc[6] = e.y; pr[7] = e.z; pc[7] = e.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool v = o0 + k < n;
        pr[k] = v ? places[2 * (o0 + k)] : (1 << 29);
        pc[k] = v ? places[2 * (o0 + k) + 1] : (1 << 29);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (pr[k] < tr0 + CT && pr[k] + cs > tr0 && pc[k] < tc0 + CT && pc[k] + cs > tc0) hits |= 1u << k;
    // exclusive prefix of the hit counts over the 256 threads: wave scan, then the wave totals through LDS
    const int cnt = __popc(hits);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (w < wave) base += s_wsum[w];
    const int total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    int pos = base + incl - cnt;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (hits & (1u << k)) {
        s_list[pos] = o0 + k;
        s_lr[pos] = pr[k];
        s_lc[pos] = pc[k];
        ++pos;
      }
    __syncthreads();
    if (total > 0) {
      if (!loaded) {
        loaded = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = tr0 + ty + 16 * (q >> 1), c = tc0 + tx + 16 * (q & 1);
          if (r < F && c < F) {
            const long e0 = ((long)r * F + c) * nb;
#pragma unroll
            for (int b = 0; b < NBMAX; ++b)
              if (b < nb) {
                am[q][b] = mean_f[e0 + b];
                as[q][b] = std_f[e0 + b];
                if (res_f) ar[q][b] = res_f[e0 + b];
                if constexpr (EPS) ae[q][b] = eps_f[e0 + b];
              }
          }
        }
      }
      for (int k = 0; k < total; ++k) {
        const int lr = s_lr[k], lc = s_lc[k];
        const long sb = (long)s_list[k] * cs;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rr = tr0 + ty + 16 * (q >> 1) - lr, cc = tc0 + tx + 16 * (q & 1) - lc;
          if ((unsigned)rr < (unsigned)cs && (unsigned)cc < (unsigned)cs) {
            const long so = ((sb + rr) * cs + cc) * nb;
            touched |= 1u << q;
#pragma unroll
            for (int b = 0; b < NBMAX; ++b)
              if (b < nb) {
                const double v = (double)loc[so + b];
                am[q][b] += v;
                ar[q][b] -= v;
                as[q][b] += (double)scale[so + b];
                if constexpr (X4 == X4_EPS) ae[q][b] += (double)eps[so + b];
                if constexpr (X4 == X4_RES2) ae[q][b] -= v;
              }
          }
        }
      }
    }
    __syncthreads();                       // the list is rewritten by the next round
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = tr0 + ty + 16 * (q >> 1), c = tc0 + tx + 16 * (q & 1);
    if ((touched >> q) & 1u) {             // (touched implies the pixel lies inside the field: windows are tested against it)
      if (r < F && c < F) {
        const long e0 = ((long)r * F + c) * nb;
#pragma unroll
        for (int b = 0; b < NBMAX; ++b)
          if (b < nb) {
            mean_f[e0 + b] = am[q][b];
            std_f[e0 + b] = as[q][b];
            if (res_f) res_f[e0 + b] = ar[q][b];
            if constexpr (EPS) eps_f[e0 + b] = ae[q][b];
          }
      }
    }
  }
}

// ---- the same at fractional positions (dv_infer_fields_fit_composite) ------------------------------------
// objs[i] of stamp i from its integer distance to the field centre and its (fitted) shift: total position dist + shift,
// top-left corner at po + that.  Both totals integer: an exact translation (coef = -1), as in scene_composite.
__global__ __launch_bounds__(256) void scene_places_kernel(const double* __restrict__ dist,
                                                           const double* __restrict__ shifts, int n, int po,
                                                           SceneObj* __restrict__ objs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double px = dist[2 * i] + shifts[2 * i], py = dist[2 * i + 1] + shifts[2 * i + 1];
  SceneObj o;
  o.sx = po + px; o.sy = po + py;
  o.ix = (int)floor(o.sx); o.iy = (int)floor(o.sy);
  o.coef = (px == floor(px) && py == floor(py)) ? -1 : 0;
  o.pad_ = 0;
  objs[i] = o;
}

// coefficients of the float32 stamps of a sub-chunk, cast exactly: coef[o][plane][P][P][nb] for the objects that are not
// exact translations; blockIdx.y = plane (mean, stddev, Monte-Carlo std)
__global__ __launch_bounds__(256) void scene_prefilter_chunk_kernel(const float* __restrict__ loc,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ eps,
                                                                    const SceneObj* __restrict__ objs, int cs, int nb,
                                                                    double* __restrict__ coef) {
  const int o = blockIdx.x, pl = blockIdx.y;
  if (objs[o].coef < 0) return;                                  // (uniform over the workgroup)
  const int P = cs + 2 * T_MARGIN;
  const float* src = pl == 0 ? loc : (pl == 1 ? scale : eps);
  scene_prefilter_body(src + (long)o * cs * cs * nb, cs, nb, coef + ((long)o * gridDim.y + pl) * P * P * nb);
}

// scene_composite_chunk_kernel for a sub-chunk of at most FSUB objects some of which sit at fractional positions: the same
// sums, order and ownership - a workgroup owns a field tile (16 x 16, one pixel per thread: the spline terms take the
// registers the other three pixels had), tests one object per thread, compacts the hits IN ORDER into an LDS list and
// walks it; float64, no atomics, load-add-store across sub-chunks and chunks, only touched pixels written, a field's
// workgroups scan that field's objects only.  An exact translation adds the float32 stamp as the integer kernel does (the
// same bits); any other object is evaluated by scene_spline_eval from the sub-chunk's coefficients, whose support
// rings T + 2 pixels beyond the stamp: the hit test uses that window.
// The sub-chunk bounds the coefficient workspace (FSUB * planes * P * P * nb doubles) whatever the chunk or the call holds.
constexpr int FT = 16;       // tile edge
constexpr int FSUB = 64;     // objects per launch
template <int NBMAX, int X4>
__global__ __launch_bounds__(256) void scene_composite_frac_kernel(double* __restrict__ mean_f, double* __restrict__ std_f,
                                                                   double* __restrict__ res_f, int F, int nb,
                                                                   const float* __restrict__ loc,
                                                                   const float* __restrict__ scale,
                                                                   const SceneObj* __restrict__ objs, int n, int cs, int po,
                                                                   const int* __restrict__ fptr, int f0, int fy0,
                                                                   long obase, double* __restrict__ eps_f,
                                                                   const float* __restrict__ eps,
                                                                   const double* __restrict__ coef) {
  __shared__ int s_list[FSUB];
  __shared__ int s_wsum[4];
  constexpr bool EPS = X4 != X4_NONE;
  constexpr int NP = X4 == X4_EPS ? 3 : 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntx = (F + FT - 1) / FT;
  const int tr0 = (blockIdx.x / ntx) * FT, tc0 = (blockIdx.x % ntx) * FT;
  const int r = tr0 + (tid >> 4), c = tc0 + (tid & 15);
  const int m = fy0 + (int)blockIdx.y;   // uniform over the workgroup
  const long lo = (long)fptr[m] - obase, hi = (long)fptr[m + 1] - obase;
  const int olo = (int)(lo > 0 ? lo : 0);
  n = (int)(hi < n ? hi : n);
  if (olo >= n) return;
  // thread t tests object olo + t (n <= FSUB <= 256: one round)
  const int o = olo + tid;
  int hit = 0;
  if (o < n) {
    const SceneObj ob = objs[o];
    const int wlo = ob.coef < 0 ? 0 : T_MARGIN + 2, whi = ob.coef < 0 ? cs : cs + T_MARGIN + 3;
    hit = ob.ix - wlo < tr0 + FT && ob.ix + whi > tr0 && ob.iy - wlo < tc0 + FT && ob.iy + whi > tc0;
  }
  int incl = hit;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < wave) base += s_wsum[w];
  const int total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
  if (hit) s_list[base + incl - 1] = o;
  __syncthreads();
  if (total == 0 || r >= F || c >= F) return;   // (no barrier below)
  const long fo = (long)(m - f0) * F * F * nb;
  const long e0 = fo + ((long)r * F + c) * nb;
  double am[NBMAX], as[NBMAX], ar[NBMAX], ae[NBMAX];
#pragma unroll
  for (int b = 0; b < NBMAX; ++b) {
    am[b] = as[b] = ar[b] = ae[b] = 0.0;
    if (b < nb) {
      am[b] = mean_f[e0 + b];
      as[b] = std_f[e0 + b];
      if (res_f) ar[b] = res_f[e0 + b];
      if constexpr (EPS) ae[b] = eps_f[e0 + b];
    }
  }
  bool touched = false;
  const long PP = (long)(cs + 2 * T_MARGIN) * (cs + 2 * T_MARGIN) * nb;
  for (int k = 0; k < total; ++k) {
    const int oo = s_list[k];
    const SceneObj ob = objs[oo];
    if (ob.coef < 0) {
      const int rr = r - ob.ix, cc = c - ob.iy;
      if ((unsigned)rr < (unsigned)cs && (unsigned)cc < (unsigned)cs) {
        const long so = (((long)oo * cs + rr) * cs + cc) * nb;
        touched = true;
#pragma unroll
        for (int b = 0; b < NBMAX; ++b)
          if (b < nb) {
            const double v = (double)loc[so + b];
            am[b] += v;
            ar[b] -= v;
            as[b] += (double)scale[so + b];
            if constexpr (X4 == X4_EPS) ae[b] += (double)eps[so + b];
            if constexpr (X4 == X4_RES2) ae[b] -= v;
          }
      }
      continue;
    }
    const double* cb = coef + (long)oo * NP * PP;
    double v[NP][NBMAX];
    bool in;
    if constexpr (NP == 3) {
      const double* const cf[3] = {cb, cb + PP, cb + 2 * PP};
      in = scene_spline_eval<3, NBMAX>(cf, nb, nb, cs, F, po, ob.sx, ob.sy, r, c, v);
    } else {
      const double* const cf[2] = {cb, cb + PP};
      in = scene_spline_eval<2, NBMAX>(cf, nb, nb, cs, F, po, ob.sx, ob.sy, r, c, v);
    }
    if (!in) continue;
    touched = true;
#pragma unroll
    for (int b = 0; b < NBMAX; ++b)
      if (b < nb) {
        am[b] += v[0][b];
        ar[b] -= v[0][b];
        as[b] += v[1][b];
        if constexpr (X4 == X4_EPS) ae[b] += v[2][b];
        if constexpr (X4 == X4_RES2) ae[b] -= v[0][b];
      }
  }
  if (!touched) return;
#pragma unroll
  for (int b = 0; b < NBMAX; ++b)
    if (b < nb) {
      mean_f[e0 + b] = am[b];
      std_f[e0 + b] = as[b];
      if (res_f) res_f[e0 + b] = ar[b];
      if constexpr (EPS) eps_f[e0 + b] = ae[b];
    }
}

// mse_center[i] = mean over the centre 10 x 10 pixels and all bands of (cutout_i - mean_i)^2 in float64
// (field_deblender.py:323-327: mse(cutout_images[k, c0:c1, c0:c1], output_images_mean[i, c0:c1, c0:c1]) with
// c0 = int(cs/2) - 5, c1 = int(cs/2) + 5; training/metrics.py:4-12); one wave per stamp.
// The 100 * nb squares are added in the order numpy's np.mean adds them (pairwise summation: halves cut at multiples of
// eight down to blocks of at most 128, a block as eight interleaved partial sums combined ((0+1)+(2+3))+((4+5)+(6+7)), then
// its tail), so the value has the bits of the reference's host formula and of DeblendField's default path.  The wave's
// lanes write the squares to LDS; lane 0 adds them (a few hundred additions per stamp).
constexpr int MSE_MAX = 100 * 8;     // squares per stamp: 10 x 10 pixels, at most 8 bands

__device__ double mse_block_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// sum(a[0..n)) in numpy's pairwise order, n <= MSE_MAX (at most three levels of halving above the 128-element blocks)
__device__ double mse_pairwise_sum(const double* a, int n) {
  int off[8], len[8], stage[8], sp = 0, vt = 0;
  double val[8];
  off[0] = 0; len[0] = n; stage[0] = 0; sp = 1;
  while (sp > 0) {
    const int t = sp - 1;
    if (len[t] <= 128) {
      val[vt++] = mse_block_sum(a + off[t], len[t]);
      --sp;
    } else if (stage[t] < 2) {
      int n2 = len[t] / 2;
      n2 -= n2 % 8;
      const int left = stage[t] == 0;
      ++stage[t];
      off[sp] = left ? off[t] : off[t] + n2;
      len[sp] = left ? n2 : len[t] - n2;
      stage[sp] = 0;
      ++sp;
    } else {
      val[vt - 2] = val[vt - 2] + val[vt - 1];
      --vt;
      --sp;
    }
  }
  return val[0];
}

// eps_norm[i] = sum(std_i[:, :, 2]) / sum(mean_i[:, :, 2]) (field_deblender.py:315-318: the Monte-Carlo std of a galaxy's
// r band over its predicted r-band flux), both sums in float64; one wave per stamp, four stamps per workgroup.  Lane l adds
// the pixels l, l + 64, ... of both stamps in that order (the band-2 element of every pixel is read once), then the 64 partial
// sums meet in a fixed shuffle tree: the same bits on every run, whatever else the chunk holds.  The division is IEEE's, so
// an all-zero mean gives numpy's inf / nan without a trap.
__global__ __launch_bounds__(256) void scene_eps_norm_kernel(const float* __restrict__ eps, const float* __restrict__ loc,
                                                             int n, int cs, int nb, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 4 + wave;
  if (i >= n) return;                                            // (uniform over the wave)
  const int px = cs * cs;
  const long base = i * px * nb + 2;
  double se = 0.0, sm = 0.0;
  for (int e = lane; e < px; e += 64) {
    se += (double)eps[base + (long)e * nb];
    sm += (double)loc[base + (long)e * nb];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    se += __shfl_down(se, d, 64);
    sm += __shfl_down(sm, d, 64);
  }
  if (lane == 0) out[i] = se / sm;
}

__global__ __launch_bounds__(256) void scene_center_mse_kernel(const double* __restrict__ field, int F, int nb,
                                                               const int* __restrict__ starts,
                                                               const float* __restrict__ loc, int n, int cs,
                                                               double* __restrict__ out,
                                                               const int* __restrict__ sfield, int f0) {
  __shared__ double s_sq[4][MSE_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  const bool valid = i < n;                                      // (uniform over the wave)
  if (valid) field += (long)(sfield[i] - f0) * F * F * nb;      // the field stamp i was cut from (uniform over the wave)
  const int c0 = cs / 2 - 5, w = 10;
  const int x0 = valid ? starts[2 * i] : 0, y0 = valid ? starts[2 * i + 1] : 0;
  const int total = w * w * nb;
  double* sq = s_sq[wave];
  for (int e = lane; valid && e < total; e += 64) {
    const int b = e % nb, q = e / nb, cc = q % w, rr = q / w;
    const double a = field[((long)(x0 + c0 + rr) * F + (y0 + c0 + cc)) * nb + b];
    const double m = (double)loc[(((long)i * cs + c0 + rr) * cs + c0 + cc) * nb + b];
    const double d = a - m;
    sq[e] = __dmul_rn(d, d);
  }
  __syncthreads();
  if (valid && lane == 0) out[i] = mse_pairwise_sum(sq, total) / (double)total;
}

// ---- resident field sets (dv_field_set_*) ---------------------------------------------------------------
// dst[m] = src[m] for the fields of a stack that have stamps in the pass (fptr[m + 1] > fptr[m]); the others are not touched.
__global__ __launch_bounds__(256) void scene_fields_copy_kernel(double* __restrict__ dst, const double* __restrict__ src,
                                                                const int* __restrict__ fptr, long felems) {
  const int m = blockIdx.y;
  if (fptr[m + 1] <= fptr[m]) return;                            // (uniform over the workgroup)
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < felems) dst[(long)m * felems + e] = src[(long)m * felems + e];
}

// field_mse[m] = mean((a[m] - b[m])^2) over the felems elements of field m, float64, for the fields that have stamps.
// A fixed decomposition, so that a field's value has the same bits on every run, for any number of fields and whatever
// the other fields hold: workgroup k of a field sums elements [k * MSE_BLK, (k + 1) * MSE_BLK) - thread t adds the squares
// of elements t, t + 256, ... of the block in that order, the 64 lanes of a wave meet in the shuffle tree (32, 16, .. 1),
// the four wave sums are added ((0 + 1) + (2 + 3)) - and writes one partial; the finish kernel (one workgroup per field)
// adds the partials the same way: thread t takes partials t, t + 256, ... in order, then the same two trees.  Every
// product and sum is rounded on its own (no contraction into FMAs).
constexpr int MSE_BLK = 2048;        // elements per workgroup: 8 per thread
__device__ __forceinline__ double field_mse_block_tree(double acc, double* s_w) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = acc;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);                  // (every thread; thread 0 stores it)
}

__global__ __launch_bounds__(256) void scene_field_mse_part_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                   const int* __restrict__ fptr, long felems, int nblk,
                                                                   double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_w[4];
  const int m = blockIdx.y;
  if (fptr[m + 1] <= fptr[m]) return;                            // (uniform over the workgroup)
  const double* fa = a + (long)m * felems;
  const double* fb = b + (long)m * felems;
  const long e0 = (long)blockIdx.x * MSE_BLK + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < MSE_BLK / 256; ++k) {
    const long e = e0 + (long)k * 256;
    if (e < felems) {
      const double d = fa[e] - fb[e];
      acc += __dmul_rn(d, d);
    }
  }
  const double tot = field_mse_block_tree(acc, s_w);
  if (threadIdx.x == 0) part[(long)m * nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void scene_field_mse_finish_kernel(const double* __restrict__ part,
                                                                     const int* __restrict__ fptr, long felems, int nblk,
                                                                     double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_w[4];
  const int m = blockIdx.x;
  if (fptr[m + 1] <= fptr[m]) return;                            // (uniform over the workgroup)
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) acc += part[(long)m * nblk + i];
  const double tot = field_mse_block_tree(acc, s_w);
  if (threadIdx.x == 0) out[m] = tot / (double)felems;
}
}  // namespace

int scene_extract(const double* field_h, int F, int nb, const int32_t* starts_h, int N, int cs, double* out_h,
                  hipStream_t s) {
  if (!field_h || !starts_h || !out_h || F < 1 || nb < 1 || cs < 1 || N < 0) {
    set_error("scene_extract: bad arguments");
    return E_INVALID;
  }
  if (N == 0) return OK;
  for (int i = 0; i < N; ++i) {
    const int x = starts_h[2 * i], y = starts_h[2 * i + 1];
    if (x < 0 || y < 0 || x > F - cs || y > F - cs) {   // (cs <= F holds; no x + cs: it overflows near INT_MAX)
      set_error("scene_extract: cutout %d (start %d,%d size %d) leaves the %d-pixel field", i, x, y, cs, F);
      return E_INVALID;
    }
  }
  const size_t fb = (size_t)F * F * nb * sizeof(double), ob = (size_t)N * cs * cs * nb * sizeof(double);
  DevBuf<double> field, out;
  DevBuf<int> starts;
  DV_TRY(field.alloc((size_t)F * F * nb));
  DV_TRY(out.alloc((size_t)N * cs * cs * nb));
  DV_TRY(starts.alloc((size_t)N * 2));
  DV_HIP(hipMemcpyAsync(field, field_h, fb, hipMemcpyHostToDevice, s));
  DV_HIP(hipMemcpyAsync(starts, starts_h, (size_t)N * 2 * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(scene_extract_kernel<double>, dim3((unsigned)N), dim3(256), 0, s, field, F, nb, starts, cs,
                     out, (const int*)nullptr, 0);
  DV_HIP(hipGetLastError());
  DV_HIP(hipMemcpyAsync(out_h, out, ob, hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  return OK;
}

int launch_scene_extract_f32(const double* field_dev, int F, int nb, const int* starts_dev, long count, int cs,
                             float* out_dev, hipStream_t s, const int* sfield_dev, int f0) {
  const long total = count * cs * cs * nb;
  if (total <= 0) return OK;
  hipLaunchKernelGGL(scene_extract_kernel<float>, dim3((unsigned)count), dim3(256), 0, s, field_dev, F, nb, starts_dev, cs,
                     out_dev, sfield_dev, f0);
  DV_HIP(hipGetLastError());
  return OK;
}

int scene_composite(double* field_h, int F, int nb, const double* stamps_h, const double* pos_h, int N, int cs,
                    double sign, hipStream_t s) {
  if (!field_h || F < 1 || nb < 1 || cs < 1 || cs > F || N < 0 || (N > 0 && (!stamps_h || !pos_h))) {
    set_error("scene_composite: bad arguments");
    return E_INVALID;
  }
  if (N == 0) return OK;
  const int P = cs + 2 * T_MARGIN;
  const int po = (F - cs) / 2;                 // int((field_size - cutout_size) / 2), field_deblender.py:70
  const int CHUNK = 256;                       // objects per pass (coefficient buffer <= 256 * P*P*nb doubles)
  const size_t fb = (size_t)F * F * nb * sizeof(double);
  const size_t stamp_elems = (size_t)cs * cs * nb;
  DevBuf<double> field, stamps, coef;     // (coef: allocated by the first chunk that has a fractional position)
  DevBuf<SceneObj> objs;
  DevBuf<int> which;
  DV_TRY(field.alloc((size_t)F * F * nb));
  DV_TRY(stamps.alloc((size_t)CHUNK * stamp_elems));
  DV_TRY(objs.alloc((size_t)CHUNK));
  DV_TRY(which.alloc((size_t)CHUNK));
  DV_HIP(hipMemcpyAsync(field, field_h, fb, hipMemcpyHostToDevice, s));
  SceneObj hobj[256];
  int hwhich[256];
  for (int base = 0; base < N; base += CHUNK) {
    const int n = N - base < CHUNK ? N - base : CHUNK;
    int nsub = 0;
    for (int i = 0; i < n; ++i) {
      const double px = pos_h[2 * (base + i)], py = pos_h[2 * (base + i) + 1];
      if (!(px == px) || !(py == py) || px > 1e9 || px < -1e9 || py > 1e9 || py < -1e9) {
        set_error("scene_composite: object %d has a non-finite position", base + i);
        return E_INVALID;
      }
      SceneObj o;
      o.sx = po + px; o.sy = po + py;
      const bool integer = px == floor(px) && py == floor(py);
      o.ix = (int)floor(o.sx); o.iy = (int)floor(o.sy);
      o.coef = integer ? -1 : nsub;
      o.pad_ = 0;
      if (!integer) hwhich[nsub++] = i;
      hobj[i] = o;
    }
    DV_HIP(hipMemcpyAsync(stamps, stamps_h + (size_t)base * stamp_elems, (size_t)n * stamp_elems * sizeof(double),
                          hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(objs, hobj, (size_t)n * sizeof(SceneObj), hipMemcpyHostToDevice, s));
    if (nsub > 0) {
      DV_TRY(coef.ensure((size_t)CHUNK * P * P * nb));
      DV_HIP(hipMemcpyAsync(which, hwhich, (size_t)nsub * sizeof(int), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(scene_prefilter_kernel, dim3(nsub), dim3(256), 0, s, stamps, which, cs, nb, coef);
      DV_HIP(hipGetLastError());
    }
    const long total = (long)F * F * nb;
    hipLaunchKernelGGL(scene_composite_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, field, F,
                       nb, stamps, coef, objs, n, cs, po, sign);
    DV_HIP(hipGetLastError());
    DV_HIP(hipStreamSynchronize(s));           // hobj / hwhich are reused by the next chunk
  }
  DV_HIP(hipMemcpyAsync(field_h, field, fb, hipMemcpyDeviceToHost, s));
  DV_HIP(hipStreamSynchronize(s));
  return OK;
}

}  // namespace dv

namespace dv {
int launch_scene_composite_chunk(double* mean_f, double* std_f, double* res_f, int F, int nb, const float* loc,
                                 const float* scale, const int* places_dev, int n, int cs, hipStream_t s,
                                 const int* fptr_dev, int f0, int fy0, int nfields, long obase, double* eps_f,
                                 const float* eps, double* res2_f) {
  if (n <= 0) return OK;
  if ((eps_f == nullptr) != (eps == nullptr)) {
    set_error("scene composite: the epistemic field and the std stamps go together");
    return E_INVALID;
  }
  if (res2_f && (eps_f || !res_f)) {
    set_error("scene composite: a second residual goes with the first and without the epistemic field");
    return E_INVALID;
  }
  if (nb < 1 || nb > 8) {
    set_error("scene composite: 1 .. 8 bands");
    return E_INVALID;
  }
  const int ntx = (F + CT - 1) / CT;
  if (nfields < 1 || nfields > 65535) {
    set_error("scene composite: a chunk spans %d fields, at most 65535", nfields);
    return E_INVALID;
  }
  const dim3 grid((unsigned)(ntx * ntx), (unsigned)nfields);
  double* x4_f = res2_f ? res2_f : eps_f;
#define SCC_LAUNCH(NBMAX, X4)                                                                                          \
  hipLaunchKernelGGL((scene_composite_chunk_kernel<NBMAX, X4>), grid, dim3(256), 0, s, mean_f, std_f, res_f, F, nb, loc, \
                     scale, places_dev, n, cs, fptr_dev, f0, fy0, obase, x4_f, eps)
  if (nb <= 6) {
    if (res2_f) SCC_LAUNCH(6, X4_RES2); else if (eps_f) SCC_LAUNCH(6, X4_EPS); else SCC_LAUNCH(6, X4_NONE);
  } else {
    if (res2_f) SCC_LAUNCH(8, X4_RES2); else if (eps_f) SCC_LAUNCH(8, X4_EPS); else SCC_LAUNCH(8, X4_NONE);
  }
#undef SCC_LAUNCH
  DV_HIP(hipGetLastError());
  return OK;
}

// doubles of coefficient workspace launch_scene_composite_frac needs (planes: 2, or 3 with the epistemic field)
size_t scene_frac_coef_doubles(int cs, int nb, int planes) {
  const size_t P = (size_t)cs + 2 * T_MARGIN;
  return (size_t)FSUB * planes * P * P * nb;
}
size_t scene_frac_obj_bytes(size_t n) { return n * sizeof(SceneObj); }

// objs_dev[i] for the n stamps of a chunk from their distances and shifts (device [n][2] each)
int launch_scene_places(const double* dist_dev, const double* shifts_dev, int n, int F, int cs, void* objs_dev,
                        hipStream_t s) {
  if (n <= 0) return OK;
  hipLaunchKernelGGL(scene_places_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dist_dev, shifts_dev, n,
                     (F - cs) / 2, static_cast<SceneObj*>(objs_dev));
  DV_HIP(hipGetLastError());
  return OK;
}

// launch_scene_composite_chunk at the placements objs_dev (launch_scene_places), FSUB objects at a time in object order:
// the sub-chunk's coefficients into coef_dev, then its sums.  sfield_h [n]: the field of every stamp of the chunk (host).
int launch_scene_composite_frac(double* mean_f, double* std_f, double* res_f, int F, int nb, const float* loc,
                                const float* scale, const void* objs_dev, int n, int cs, hipStream_t s, const int* fptr_dev,
                                int f0, const int32_t* sfield_h, long obase, double* eps_f, const float* eps,
                                double* res2_f, double* coef_dev) {
  if (n <= 0) return OK;
  if ((eps_f == nullptr) != (eps == nullptr)) {
    set_error("scene composite: the epistemic field and the std stamps go together");
    return E_INVALID;
  }
  if (res2_f && (eps_f || !res_f)) {
    set_error("scene composite: a second residual goes with the first and without the epistemic field");
    return E_INVALID;
  }
  if (nb < 1 || nb > 8 || cs > F || !coef_dev || !objs_dev) {
    set_error("scene composite: 1 .. 8 bands, stamps within the field, a coefficient workspace");
    return E_INVALID;
  }
  const int ntx = (F + FT - 1) / FT, po = (F - cs) / 2;
  const int planes = eps_f ? 3 : 2;
  const size_t stamp = (size_t)cs * cs * nb;
  double* x4_f = res2_f ? res2_f : eps_f;
  const SceneObj* objs = static_cast<const SceneObj*>(objs_dev);
  for (int a = 0; a < n; a += FSUB) {
    const int ns = n - a < FSUB ? n - a : FSUB;
    const int fy0 = sfield_h[a], nfields = sfield_h[a + ns - 1] - fy0 + 1;
    if (nfields < 1 || nfields > 65535) {
      set_error("scene composite: a sub-chunk spans %d fields, at most 65535", nfields);
      return E_INVALID;
    }
    const float* l = loc + (size_t)a * stamp;
    const float* sc = scale + (size_t)a * stamp;
    const float* ep = eps ? eps + (size_t)a * stamp : nullptr;
    hipLaunchKernelGGL(scene_prefilter_chunk_kernel, dim3((unsigned)ns, (unsigned)planes), dim3(256), 0, s, l, sc, ep,
                       objs + a, cs, nb, coef_dev);
    DV_HIP(hipGetLastError());
    const dim3 grid((unsigned)(ntx * ntx), (unsigned)nfields);
#define SCF_LAUNCH(NBMAX, X4)                                                                                            \
  hipLaunchKernelGGL((scene_composite_frac_kernel<NBMAX, X4>), grid, dim3(256), 0, s, mean_f, std_f, res_f, F, nb, l, sc, \
                     objs + a, ns, cs, po, fptr_dev, f0, fy0, obase + a, x4_f, ep, coef_dev)
    if (nb <= 6) {
      if (res2_f) SCF_LAUNCH(6, X4_RES2); else if (eps_f) SCF_LAUNCH(6, X4_EPS); else SCF_LAUNCH(6, X4_NONE);
    } else {
      if (res2_f) SCF_LAUNCH(8, X4_RES2); else if (eps_f) SCF_LAUNCH(8, X4_EPS); else SCF_LAUNCH(8, X4_NONE);
    }
#undef SCF_LAUNCH
    DV_HIP(hipGetLastError());
  }
  return OK;
}

int launch_scene_eps_norm(const float* eps, const float* loc, int n, int cs, int nb, double* out_dev, hipStream_t s) {
  if (n <= 0) return OK;
  if (nb < 3 || cs < 1) {
    set_error("normalised epistemic uncertainty: band 2 of stamps with at least 3 bands");
    return E_INVALID;
  }
  hipLaunchKernelGGL(scene_eps_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, eps, loc, n, cs, nb, out_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_scene_fields_copy(double* dst_dev, const double* src_dev, const int* fptr_dev, int M, long felems,
                             hipStream_t s) {
  if (M <= 0 || felems <= 0) return OK;
  if (M > 65535) {
    set_error("field set: %d fields, at most 65535", M);
    return E_INVALID;
  }
  hipLaunchKernelGGL(scene_fields_copy_kernel, dim3((unsigned)((felems + 255) / 256), (unsigned)M), dim3(256), 0, s, dst_dev,
                     src_dev, fptr_dev, felems);
  DV_HIP(hipGetLastError());
  return OK;
}

long scene_field_mse_blocks(long felems) { return (felems + MSE_BLK - 1) / MSE_BLK; }

int launch_scene_field_mse(const double* a_dev, const double* b_dev, const int* fptr_dev, int M, long felems,
                           double* part_dev, double* out_dev, hipStream_t s) {
  if (M <= 0 || felems <= 0) return OK;
  const long nblk = scene_field_mse_blocks(felems);
  if (M > 65535 || nblk > 0x7fffffffL) {
    set_error("field set: %d fields of %ld elements are beyond the reduction's grid", M, felems);
    return E_INVALID;
  }
  hipLaunchKernelGGL(scene_field_mse_part_kernel, dim3((unsigned)nblk, (unsigned)M), dim3(256), 0, s, a_dev, b_dev, fptr_dev,
                     felems, (int)nblk, part_dev);
  DV_HIP(hipGetLastError());
  hipLaunchKernelGGL(scene_field_mse_finish_kernel, dim3((unsigned)M), dim3(256), 0, s, part_dev, fptr_dev, felems, (int)nblk,
                     out_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_scene_center_mse(const double* field_dev, int F, int nb, const int* starts_dev, const float* loc, int n, int cs,
                            double* out_dev, hipStream_t s, const int* sfield_dev, int f0) {
  if (n <= 0) return OK;
  if (cs < 10) {
    set_error("centre MSE needs stamps of at least 10 pixels");
    return E_INVALID;
  }
  if (nb < 1 || nb > 8) {
    set_error("centre MSE: 1 .. 8 bands");
    return E_INVALID;
  }
  hipLaunchKernelGGL(scene_center_mse_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, field_dev, F, nb, starts_dev, loc,
                     n, cs, out_dev, sfield_dev, f0);
  DV_HIP(hipGetLastError());
  return OK;
}
}  // namespace dv
