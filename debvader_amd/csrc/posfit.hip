// Sub-pixel position fit (reference: deblend_cutout/optimization.py, position_optimization), batched over galaxies.
//
// Reference behaviour restated, per galaxy (r band only, F = field size, po = int((F - cs) / 2)):
//   net  = shift(pad(stamp), d)                     pad(): the cs x cs stamp centred at po in a zero F x F image
//   J(s) = mean over all F*F pixels of (img - shift(net, s))^2
//   s*   = argmin J over s in [-bound, bound]^2, started from the given shifts (zeros in the reference)
// where shift() is scipy.ndimage.shift with its defaults (cubic B-spline, mode "constant": the coefficients are those of the
// image mirrored at its edge samples, an output pixel whose input coordinate leaves [0, F-1] is 0).  The reference runs
// scipy.optimize.least_squares with a 2-point Jacobian on each galaxy in a Python loop.
//
// Here: one workgroup per galaxy, float64 throughout.
//  1. Coefficients.  For a mirror-extended image ext (ext[i] = img[reflect(i)]) the spline coefficients are the infinite-
//     domain recursive prefilter (pole sqrt(3) - 2) of ext, and they are themselves mirror symmetric, so the coefficient a
//     tap k in [-1, F+1] of scipy's evaluation reads (the mirrored one) is c_ext[k].  The workgroup computes c_ext only on
//     the window of taps the fit can touch, running the recursion T = 20 samples beyond it on each side from zero
//     (0.268^20 = 4e-12, the T_MARGIN of scene.hip).  An integer d makes net an exact translation of the stamp; a
//     fractional d first builds the coefficients of pad() the same way and evaluates net from them on the stamp's
//     footprint plus T + 2 pixels (beyond it net is below 4e-12 of the stamp), so the two interpolations compose as in
//     the reference.
//  2. Objective.  shift(net, s) is significant only on the window E = net's support + T + ceil(bound) + 2; pixels outside
//     it contribute img^2, a per-galaxy constant (sum over the field minus the sum over E).  One pass over E returns J, the
//     gradient and the 2 x 2 Hessian: the shift is the same for every pixel, so the 4 x 4 B-spline weights and their first
//     and second derivatives are computed once per pass and the derivatives of J follow analytically (no finite
//     differences).  Per pixel: 16 coefficient loads, ~70 FMAs.  Reductions go butterfly within a wave, then through LDS in
//     wave order: bit-reproducible, independent of how galaxies are batched.
//  3. Optimiser.  Box-projected Newton with Levenberg damping: coordinates on a bound whose gradient points outwards are
//     held, the free ones take a damped Newton step, the step is projected into [-bound, bound]^2 and accepted when J
//     decreases (or, within rounding of J, when the projected gradient shrinks); otherwise the damping grows.  Stops when
//     the step or the projected gradient is below 1e-10 px (status 0, or 1 on a bound), at max_iter (2), or when no damped
//     step lowers J (3, stalled).  Every thread runs the same scalar logic on the
//     reduced values, so there is no divergence and no broadcast.
// fp64 VALU work; nothing here has a matrix shape for MFMA.
#include "common.h"

namespace dv {

namespace {
constexpr int PF_T = 20;                  // recursion margin (as T_MARGIN of scene.hip)
constexpr int PF_THREADS = 256;
constexpr double PF_Z1 = -0.26794919243112270647;   // sqrt(3) - 2

// per-galaxy geometry, computed on the host; windows are [lo, lo + n) in field coordinates (rows r, columns c)
struct PosfitGeom {
  double dr, dc;       // distance to the centre (net = shift(pad(stamp), d))
  double s0r, s0c;     // start shifts
  long ws;             // offset of this galaxy's workspace in doubles
  int stamp;           // stamp index within the chunk
  int field;           // the galaxy's field within the resident stack of fields (0 for a single field)
  int integer;         // 1: d is integer, net is a translation
  int empty;           // 1: net is zero everywhere (the stamp misses the field)
  int nr_lo, nr_n, nc_lo, nc_n;   // net support
  int k1r_lo, k1r_n, k1c_lo, k1c_n;   // taps of pad's coefficients (fractional d)
  int er_lo, er_n, ec_lo, ec_n;   // evaluation window
  int kr_lo, kr_n, kc_lo, kc_n;   // taps of net's coefficients
  long o_cnet, o_cpad, o_net;     // workspace offsets (doubles) after the recursion scratch at 0
};

__device__ __forceinline__ int pf_reflect(int i, int F) {
  if (F == 1) return 0;
  const int p = 2 * F - 2;
  i %= p;
  if (i < 0) i += p;
  return i >= F ? p - i : i;
}

__device__ __forceinline__ void pf_weights(double t, double w[4], double w1[4], double w2[4]) {
  const double u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
  w[2] = (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0;
  w[3] = t * t * t / 6.0;
  w1[0] = -0.5 * u * u;
  w1[1] = 1.5 * t * t - 2.0 * t;
  w1[2] = -1.5 * t * t + t + 0.5;
  w1[3] = 0.5 * t * t;
  w2[0] = u;
  w2[1] = 3.0 * t - 2.0;
  w2[2] = 1.0 - 3.0 * t;
  w2[3] = t;
}

// c[rn][cn] = coefficients of the mirror-extended image src at taps [rlo, rlo + rn) x [clo, clo + cn) (unreflected
// indices), via the recursion over the window widened by PF_T on every side; tmp holds (rn + 2T) x (cn + 2T)
template <typename SRC>
__device__ void pf_prefilter(SRC src, int rlo, int rn, int clo, int cn, double* __restrict__ tmp, double* __restrict__ c) {
  const int RW = rn + 2 * PF_T, CW = cn + 2 * PF_T;
  // axis 0 for every column of the widened window (a thread per column: coalesced along rows of tmp)
  for (int jj = threadIdx.x; jj < CW; jj += PF_THREADS) {
    const int j = clo - PF_T + jj;
    double acc = 0.0;
    for (int ii = 0; ii < RW; ++ii) {
      acc = 6.0 * src(rlo - PF_T + ii, j) + PF_Z1 * acc;
      tmp[(long)ii * CW + jj] = acc;
    }
    double nxt = 0.0;
    for (int ii = RW - 1; ii >= 0; --ii) {
      nxt = PF_Z1 * (nxt - tmp[(long)ii * CW + jj]);
      tmp[(long)ii * CW + jj] = nxt;
    }
  }
  __syncthreads();
  // axis 1 for the rows that are kept
  for (int ii = threadIdx.x; ii < rn; ii += PF_THREADS) {
    double* row = tmp + (long)(ii + PF_T) * CW;
    double acc = 0.0;
    for (int jj = 0; jj < CW; ++jj) {
      acc = 6.0 * row[jj] + PF_Z1 * acc;
      row[jj] = acc;
    }
    double nxt = 0.0;
    for (int jj = CW - 1; jj >= 0; --jj) {
      nxt = PF_Z1 * (nxt - row[jj]);
      if (jj >= PF_T && jj < PF_T + cn) c[(long)ii * cn + jj - PF_T] = nxt;
      row[jj] = nxt;
    }
  }
  __syncthreads();
}

// sum of v over the workgroup, the same order on every call; every thread gets the result
template <int K>
__device__ __forceinline__ void pf_block_sum(double (&v)[K], double* s_red) {
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

struct PfEval {
  double J, gr, gc, hrr, hrc, hcc;
};

// J, gradient and Hessian at shift (sr, sc) over the evaluation window; cst = sum of img^2 outside it
__device__ PfEval pf_eval(const double* __restrict__ img, int F, const PosfitGeom& g, const double* __restrict__ cnet,
                          double cst, double sr, double sc, double* s_red) {
  const double nsr = -sr, nsc = -sc;
  const double fr = floor(nsr), fc = floor(nsc);
  double wr[4], wr1[4], wr2[4], wc[4], wc1[4], wc2[4];
  pf_weights(nsr - fr, wr, wr1, wr2);
  pf_weights(nsc - fc, wc, wc1, wc2);
  const int ofr = (int)fr - 1 - g.kr_lo, ofc = (int)fc - 1 - g.kc_lo;   // tap row of pixel x: x + ofr (local to cnet)
  const int kcn = g.kc_n;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // r^2, r g_u, r g_v, g_u^2 - r g_uu, g_u g_v - r g_uv, g_v^2 - r g_vv
  const int total = g.er_n * g.ec_n;
  const int step_r = PF_THREADS / g.ec_n, step_c = PF_THREADS - step_r * g.ec_n;
  int pr = threadIdx.x / g.ec_n, pc = threadIdx.x - pr * g.ec_n;
  for (int e = threadIdx.x; e < total; e += PF_THREADS) {
    const int x = g.er_lo + pr, y = g.ec_lo + pc;
    const double v = img[(long)x * F + y];
    const double ur = (double)x - sr, uc = (double)y - sc;
    double val = 0.0, gu = 0.0, gv = 0.0, guu = 0.0, guv = 0.0, gvv = 0.0;
    if (ur >= 0.0 && uc >= 0.0 && ur <= F - 1.0 && uc <= F - 1.0) {
      const double* cp = cnet + (long)(x + ofr) * kcn + (y + ofc);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double* row = cp + (long)a * kcn;
        const double c0 = row[0], c1 = row[1], c2 = row[2], c3 = row[3];
        const double r0 = c0 * wc[0] + c1 * wc[1] + c2 * wc[2] + c3 * wc[3];
        const double r1 = c0 * wc1[0] + c1 * wc1[1] + c2 * wc1[2] + c3 * wc1[3];
        const double r2 = c0 * wc2[0] + c1 * wc2[1] + c2 * wc2[2] + c3 * wc2[3];
        val += wr[a] * r0;
        gu += wr1[a] * r0;
        guu += wr2[a] * r0;
        gv += wr[a] * r1;
        guv += wr1[a] * r1;
        gvv += wr[a] * r2;
      }
    }
    const double r = v - val;
    acc[0] += r * r;
    acc[1] += r * gu;
    acc[2] += r * gv;
    acc[3] += gu * gu - r * guu;
    acc[4] += gu * gv - r * guv;
    acc[5] += gv * gv - r * gvv;
    pc += step_c;
    pr += step_r;
    if (pc >= g.ec_n) { pc -= g.ec_n; ++pr; }
  }
  pf_block_sum<6>(acc, s_red);
  const double inv = 1.0 / ((double)F * (double)F);
  PfEval out;
  out.J = (cst + acc[0]) * inv;
  out.gr = 2.0 * inv * acc[1];      // dJ/ds_r: d(shift(net, s))/ds_r = -g_u
  out.gc = 2.0 * inv * acc[2];
  out.hrr = 2.0 * inv * acc[3];
  out.hrc = 2.0 * inv * acc[4];
  out.hcc = 2.0 * inv * acc[5];
  return out;
}

// a coordinate is held when it sits on a bound and the gradient points out of the box
__device__ __forceinline__ bool pf_held(double s, double grad, double B) { return (s <= -B && grad > 0.0) || (s >= B && grad < 0.0); }

// box-projected gradient: zero on the held coordinates
__device__ __forceinline__ void pf_projected(const PfEval& e, double sr, double sc, double B, double& pr, double& pc) {
  pr = pf_held(sr, e.gr, B) ? 0.0 : e.gr;
  pc = pf_held(sc, e.gc, B) ? 0.0 : e.gc;
}

// img: the resident stack of r-band fields [G][F][F], total_sq [G] their sums of squares; galaxy gi reads field geoms[gi].field
__global__ __launch_bounds__(PF_THREADS) void posfit_kernel(const double* __restrict__ img, int F,
                                                            const double* __restrict__ stamps, int cs,
                                                            const PosfitGeom* __restrict__ geoms,
                                                            double* __restrict__ work, const double* __restrict__ total_sq,
                                                            double bound, int max_iter, double* __restrict__ shifts,
                                                            double* __restrict__ objective, int* __restrict__ iters,
                                                            int* __restrict__ status) {
  __shared__ double s_red[4 * 6];
  const int gi = blockIdx.x;
  const PosfitGeom g = geoms[gi];
  img += (long)g.field * F * F;
  const double tot = total_sq[g.field];
  const double inv = 1.0 / ((double)F * (double)F);
  if (g.empty) {                      // net = 0: J is constant, nothing to fit
    if (threadIdx.x == 0) {
      shifts[2 * gi] = max_iter > 0 ? fmin(fmax(g.s0r, -bound), bound) : g.s0r;
      shifts[2 * gi + 1] = max_iter > 0 ? fmin(fmax(g.s0c, -bound), bound) : g.s0c;
      objective[gi] = tot * inv;
      iters[gi] = 0;
      status[gi] = max_iter > 0 ? 0 : 2;
    }
    return;
  }
  double* ws = work + g.ws;
  double* tmp = ws;
  double* cnet = ws + g.o_cnet;
  const double* st = stamps + (long)g.stamp * cs * cs;
  const int po = (F - cs) / 2;

  if (g.integer) {
    const int ir = (int)g.dr + po, ic = (int)g.dc + po;     // stamp's top-left corner in the field
    const int nr0 = g.nr_lo, nr1 = g.nr_lo + g.nr_n, nc0 = g.nc_lo, nc1 = g.nc_lo + g.nc_n;
    pf_prefilter([=](int i, int j) {
      i = pf_reflect(i, F);
      j = pf_reflect(j, F);
      return (i >= nr0 && i < nr1 && j >= nc0 && j < nc1) ? st[(long)(i - ir) * cs + (j - ic)] : 0.0;
    }, g.kr_lo, g.kr_n, g.kc_lo, g.kc_n, tmp, cnet);
  } else {
    double* cpad = ws + g.o_cpad;
    double* net = ws + g.o_net;
    // coefficients of pad(stamp) at the taps net's window reads
    pf_prefilter([=](int i, int j) {
      i = pf_reflect(i, F) - po;
      j = pf_reflect(j, F) - po;
      return ((unsigned)i < (unsigned)cs && (unsigned)j < (unsigned)cs) ? st[(long)i * cs + j] : 0.0;
    }, g.k1r_lo, g.k1r_n, g.k1c_lo, g.k1c_n, tmp, cpad);
    // net = shift(pad, d) on its support window
    {
      const double fr = floor(-g.dr), fc = floor(-g.dc);
      double wr[4], wc[4], t1[4], t2[4];
      pf_weights(-g.dr - fr, wr, t1, t2);
      pf_weights(-g.dc - fc, wc, t1, t2);
      const int ofr = (int)fr - 1 - g.k1r_lo, ofc = (int)fc - 1 - g.k1c_lo;
      const int total = g.nr_n * g.nc_n;
      for (int e = threadIdx.x; e < total; e += PF_THREADS) {
        const int pr = e / g.nc_n, pc = e - pr * g.nc_n;
        const int x = g.nr_lo + pr, y = g.nc_lo + pc;
        const double ur = (double)x - g.dr, uc = (double)y - g.dc;
        double v = 0.0;
        if (ur >= 0.0 && uc >= 0.0 && ur <= F - 1.0 && uc <= F - 1.0) {
          const double* cp = cpad + (long)(x + ofr) * g.k1c_n + (y + ofc);
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double* row = cp + (long)a * g.k1c_n;
            v += wr[a] * (row[0] * wc[0] + row[1] * wc[1] + row[2] * wc[2] + row[3] * wc[3]);
          }
        }
        net[e] = v;
      }
    }
    __syncthreads();
    const int nr0 = g.nr_lo, nr1 = g.nr_lo + g.nr_n, nc0 = g.nc_lo, nc1 = g.nc_lo + g.nc_n, ncn = g.nc_n;
    pf_prefilter([=](int i, int j) {
      i = pf_reflect(i, F);
      j = pf_reflect(j, F);
      return (i >= nr0 && i < nr1 && j >= nc0 && j < nc1) ? net[(long)(i - nr0) * ncn + (j - nc0)] : 0.0;
    }, g.kr_lo, g.kr_n, g.kc_lo, g.kc_n, tmp, cnet);
  }

  // the pixels outside the evaluation window contribute img^2 whatever the shift
  double cst;
  {
    double a[1] = {0.0};
    const int total = g.er_n * g.ec_n;
    for (int e = threadIdx.x; e < total; e += PF_THREADS) {
      const int pr = e / g.ec_n, pc = e - pr * g.ec_n;
      const double v = img[(long)(g.er_lo + pr) * F + g.ec_lo + pc];
      a[0] += v * v;
    }
    pf_block_sum<1>(a, s_red);
    cst = tot - a[0];
  }

  const double B = bound;
  double sr = g.s0r, sc = g.s0c;
  if (max_iter > 0) {
    sr = fmin(fmax(sr, -B), B);
    sc = fmin(fmax(sc, -B), B);
  }
  PfEval cur = pf_eval(img, F, g, cnet, cst, sr, sc, s_red);
  int it = 0, st_code = 2;
  double lam = 0.0;
  while (it < max_iter) {
    double pr, pc;
    pf_projected(cur, sr, sc, B, pr, pc);
    if (pr == 0.0 && pc == 0.0) { st_code = 0; break; }
    const bool fr_free = !pf_held(sr, cur.gr, B), fc_free = !pf_held(sc, cur.gc, B);
    const double hscale = fabs(cur.hrr) + fabs(cur.hcc) + 1e-300;
    double lt = lam;
    bool accepted = false, done = false;
    int rejected = 0;                       // trial steps that were evaluated and did not lower J
    for (int trial = 0; trial < 60; ++trial) {
      // damped Newton step on the free coordinates
      const double a = fr_free ? cur.hrr + lt : 1.0, c = fc_free ? cur.hcc + lt : 1.0;
      const double b = (fr_free && fc_free) ? cur.hrc : 0.0;
      const double det = a * c - b * b;
      if (!(a > 0.0 && c > 0.0 && det > 1e-14 * a * c)) {      // not positive definite: damp more
        lt = fmax(4.0 * lt, 1e-3 * hscale);
        continue;
      }
      const double dr = fr_free ? -(c * pr - b * pc) / det : 0.0;
      const double dc = fc_free ? -(a * pc - b * pr) / det : 0.0;
      const double nr = fmin(fmax(sr + dr, -B), B), nc = fmin(fmax(sc + dc, -B), B);
      const double stepr = nr - sr, stepc = nc - sc;
      if (fmax(fabs(stepr), fabs(stepc)) <= 1e-10) { done = true; break; }
      const PfEval nxt = pf_eval(img, F, g, cnet, cst, nr, nc, s_red);
      double npr, npc;
      pf_projected(nxt, nr, nc, B, npr, npc);
      const bool better = nxt.J < cur.J ||
          (nxt.J <= cur.J + 1e-13 * fabs(cur.J) && fmax(fabs(npr), fabs(npc)) < fmax(fabs(pr), fabs(pc)));
      if (better) {
        sr = nr;
        sc = nc;
        cur = nxt;
        ++it;
        accepted = true;
        lam = lt * 0.25 < 1e-6 * hscale ? 0.0 : lt * 0.25;
        if (fmax(fabs(stepr), fabs(stepc)) <= 1e-10) done = true;
        break;
      }
      ++rejected;
      lt = fmax(4.0 * lt, 1e-3 * hscale);
    }
    // a step below 1e-10 px is convergence only when the damping did not shrink it there after rejected steps; a line
    // search that found no lower J is reported as stalled (the shift is the best one found)
    if (done) { st_code = rejected > 0 && !accepted ? 3 : 0; break; }
    if (!accepted) { st_code = 3; break; }
  }
  if (st_code == 0 && max_iter > 0 && (fabs(sr) >= B || fabs(sc) >= B)) st_code = 1;
  if (threadIdx.x == 0) {
    shifts[2 * gi] = sr;
    shifts[2 * gi + 1] = sc;
    objective[gi] = cur.J;
    iters[gi] = it;
    status[gi] = st_code;
  }
}

// sum of img^2 over a field of n elements, one workgroup per field of the stack, fixed order
__global__ __launch_bounds__(PF_THREADS) void posfit_total_sq_kernel(const double* __restrict__ img, long n,
                                                                     double* __restrict__ out) {
  __shared__ double s_red[4];
  img += (long)blockIdx.x * n;
  double a[1] = {0.0};
  for (long e = threadIdx.x; e < n; e += PF_THREADS) a[0] += img[e] * img[e];
  pf_block_sum<1>(a, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = a[0];
}

// [lo, hi) intersected with [0, F) -> (lo, n); n = 0 if empty
void pf_clip(long lo, long hi, int F, int& olo, int& on) {
  if (lo < 0) lo = 0;
  if (hi > F) hi = F;
  olo = (int)lo;
  on = hi > lo ? (int)(hi - lo) : 0;
}

// dst[e] = band `band` of pixel e of src [npix][nb], as float64 (exact for float32 sources): the contiguous r-band planes
// and stamps posfit_kernel reads, gathered from fields and network outputs that lie in device memory
template <typename T>
__global__ __launch_bounds__(PF_THREADS) void posfit_band_kernel(const T* __restrict__ src, long npix, int nb, int band,
                                                                 double* __restrict__ dst) {
  const long e = (long)blockIdx.x * PF_THREADS + threadIdx.x;
  if (e < npix) dst[e] = (double)src[e * nb + band];
}
}  // namespace

// ---- geometry and launch layout, shared by the host-stamp calls and the device-resident stage -------------------------
struct PosfitLaunch {
  int base, n;         // galaxies base .. base + n of the plan
  long work;           // doubles of workspace
};

struct PosfitPlan {
  int F = 0, cs = 0, max_iter = 0;
  double bound = 0.0;
  std::vector<PosfitGeom> geo;
  std::vector<long> need;              // workspace doubles per galaxy
  std::vector<PosfitLaunch> launches;  // in galaxy order
  long work_max = 0;                   // the largest launch's workspace
  DevBuf<PosfitGeom> geo_dev;          // posfit_plan_upload
};

static const int PF_CHUNK = 512;                  // galaxies per launch
static const long PF_WS_BUDGET = 128L << 20;      // workspace doubles per launch (1 GiB); no galaxy may need more

void posfit_plan_destroy(PosfitPlan* p) { delete p; }

// windows and workspace need of every galaxy; refuses what dv_scene_fit_shifts refuses
int posfit_plan_create(int F, int cs, int N, const double* dist_h, const double* shifts_h, double bound, int max_iter,
                       PosfitPlan** out) {
  if (!out || F < 2 || F > 32768 || cs < 1 || cs > F || N < 0 || max_iter < 0 || !(bound >= 0.0) || bound > 1e6 ||
      (N > 0 && (!dist_h || !shifts_h))) {
    set_error("scene_fit_shifts: bad arguments");
    return E_INVALID;
  }
  const int T = PF_T;
  const int po = (F - cs) / 2;
  PosfitPlan* plan = new PosfitPlan();
  plan->F = F; plan->cs = cs; plan->max_iter = max_iter; plan->bound = bound;
  std::vector<PosfitGeom>& geo = plan->geo;
  std::vector<long>& need = plan->need;
  geo.resize((size_t)N);
  need.resize((size_t)N);
  for (int i = 0; i < N; ++i) {
    const double d[2] = {dist_h[2 * i], dist_h[2 * i + 1]}, s0[2] = {shifts_h[2 * i], shifts_h[2 * i + 1]};
    for (int k = 0; k < 2; ++k) {
      if (!(d[k] == d[k]) || d[k] > 1e6 || d[k] < -1e6 || !(s0[k] == s0[k]) || s0[k] > 1e6 || s0[k] < -1e6) {
        set_error("scene_fit_shifts: galaxy %d has a non-finite or out-of-range distance or start shift", i);
        delete plan;
        return E_INVALID;
      }
    }
    PosfitGeom g{};
    g.dr = d[0]; g.dc = d[1]; g.s0r = s0[0]; g.s0c = s0[1];
    g.stamp = 0;
    g.integer = d[0] == floor(d[0]) && d[1] == floor(d[1]);
    // reach of the shift: the box, or the start itself when only the objective is evaluated there.  Capped at F: a pixel
    // x in [0, F-1] reads taps only when x - s lies in [0, F-1], i.e. |s| <= F - 1, so floor(-s) stays within [-R, R]
    // for every pixel that reads one, and a larger shift reads none (shift(net, s) = 0, J = mean(field^2))
    double reach = bound;
    if (max_iter == 0) reach = std::max(reach, std::max(fabs(s0[0]), fabs(s0[1])));
    const long R = std::min((long)ceil(reach), (long)F);
    int nlo[2], nn[2], k1lo[2] = {0, 0}, k1n[2] = {0, 0}, elo[2], en[2], klo[2], kn[2];
    for (int k = 0; k < 2; ++k) {
      const long fd = (long)floor(d[k]);
      if (g.integer) pf_clip(po + fd, po + fd + cs, F, nlo[k], nn[k]);
      else pf_clip(po + fd - T - 2, po + fd + cs + T + 3, F, nlo[k], nn[k]);
    }
    g.empty = nn[0] == 0 || nn[1] == 0;
    long w = 0;
    if (!g.empty) {
      for (int k = 0; k < 2; ++k) {
        if (!g.integer) {
          const long fm = (long)floor(-d[k]);
          k1lo[k] = (int)(nlo[k] + fm - 1);
          k1n[k] = nn[k] + 3;
        }
        pf_clip((long)nlo[k] - T - R - 2, (long)nlo[k] + nn[k] + T + R + 2, F, elo[k], en[k]);
        klo[k] = elo[k] - (int)R - 1;
        kn[k] = en[k] + 2 * (int)R + 3;
      }
      g.nr_lo = nlo[0]; g.nr_n = nn[0]; g.nc_lo = nlo[1]; g.nc_n = nn[1];
      g.k1r_lo = k1lo[0]; g.k1r_n = k1n[0]; g.k1c_lo = k1lo[1]; g.k1c_n = k1n[1];
      g.er_lo = elo[0]; g.er_n = en[0]; g.ec_lo = elo[1]; g.ec_n = en[1];
      g.kr_lo = klo[0]; g.kr_n = kn[0]; g.kc_lo = klo[1]; g.kc_n = kn[1];
      const long tmp_n = std::max((long)(kn[0] + 2 * T) * (kn[1] + 2 * T),
                                  g.integer ? 0L : (long)(k1n[0] + 2 * T) * (k1n[1] + 2 * T));
      w = tmp_n;
      g.o_cnet = w;  w += (long)kn[0] * kn[1];
      if (!g.integer) {
        g.o_cpad = w;  w += (long)k1n[0] * k1n[1];
        g.o_net = w;   w += (long)nn[0] * nn[1];
      }
    }
    if (w > PF_WS_BUDGET) {
      set_error("scene_fit_shifts: galaxy %d needs %ld doubles of workspace, above the %ld of one launch", i, w, PF_WS_BUDGET);
      delete plan;
      return E_INVALID;
    }
    geo[i] = g;
    need[i] = w;
  }
  *out = plan;
  return OK;
}

// the workspace loop: galaxies [a, b) go into launches of as many as max_n (at most PF_CHUNK) and the workspace budget
// allow.  A galaxy reads field sfield[i] - f0 of the resident planes and stamp i - stamp0 of the resident stamps (stamp0 < 0:
// the stamps of each launch are resident on their own, stamp i - its launch's base).  Returns the index of the first launch.
int posfit_plan_layout(PosfitPlan* p, int a, int b, int max_n, const int32_t* sfield, int f0, int stamp0) {
  const int first = (int)p->launches.size();
  max_n = std::max(1, std::min(max_n, PF_CHUNK));
  for (int base = a; base < b;) {
    int n = 0;
    long w = 0;
    while (base + n < b && n < max_n && w + p->need[base + n] <= PF_WS_BUDGET) {   // (need <= PF_WS_BUDGET: n >= 1)
      PosfitGeom& g = p->geo[base + n];
      g.field = sfield[base + n] - f0;
      g.stamp = stamp0 < 0 ? n : base + n - stamp0;
      g.ws = w;
      w += p->need[base + n];
      ++n;
    }
    p->launches.push_back({base, n, w});
    p->work_max = std::max(p->work_max, w);
    base += n;
  }
  return first;
}

// the planes a group holds start at field f0: galaxies [a, b), laid out against field 0, read field sfield - f0
void posfit_plan_rebase(PosfitPlan* p, int a, int b, int f0) {
  for (int i = a; i < b; ++i) p->geo[i].field -= f0;
}

int posfit_plan_launch_count(const PosfitPlan* p) { return (int)p->launches.size(); }
long posfit_plan_work_doubles(const PosfitPlan* p) { return std::max(p->work_max, 1L); }

// the laid-out geometry of all galaxies to the device (the device-resident stage: one upload per call)
int posfit_plan_upload(PosfitPlan* p, hipStream_t s) {
  const size_t n = p->geo.size();
  if (n == 0 || p->geo_dev) return OK;
  DV_TRY(p->geo_dev.alloc(n));
  DV_HIP(hipMemcpyAsync(p->geo_dev, p->geo.data(), n * sizeof(PosfitGeom), hipMemcpyHostToDevice, s));
  return OK;
}
size_t posfit_plan_geom_bytes(size_t n) { return n * sizeof(PosfitGeom); }

// launches [l0, l1) of an uploaded plan on device-resident planes, stamps and outputs ([N] arrays indexed by galaxy)
int posfit_plan_run(const PosfitPlan* p, int l0, int l1, const double* img_dev, const double* total_sq_dev,
                    const double* stamps_dev, double* work_dev, double* shifts_dev, double* objective_dev, int* iters_dev,
                    int* status_dev, hipStream_t s) {
  for (int l = l0; l < l1; ++l) {
    const PosfitLaunch& L = p->launches[l];
    hipLaunchKernelGGL(posfit_kernel, dim3((unsigned)L.n), dim3(PF_THREADS), 0, s, img_dev, p->F, stamps_dev, p->cs,
                       p->geo_dev.get() + L.base, work_dev, total_sq_dev, p->bound, p->max_iter, shifts_dev + 2 * (size_t)L.base,
                       objective_dev + L.base, iters_dev + L.base, status_dev + L.base);
    DV_HIP(hipGetLastError());
  }
  return OK;
}

int launch_posfit_total_sq(const double* img_dev, int nfields, long elems, double* out_dev, hipStream_t s) {
  if (nfields <= 0) return OK;
  hipLaunchKernelGGL(posfit_total_sq_kernel, dim3((unsigned)nfields), dim3(PF_THREADS), 0, s, img_dev, elems, out_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_posfit_band_f64(const double* src_dev, long npix, int nb, int band, double* dst_dev, hipStream_t s) {
  if (npix <= 0) return OK;
  hipLaunchKernelGGL(posfit_band_kernel<double>, dim3((unsigned)((npix + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0,
                     s, src_dev, npix, nb, band, dst_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int launch_posfit_band_f32(const float* src_dev, long npix, int nb, int band, double* dst_dev, hipStream_t s) {
  if (npix <= 0) return OK;
  hipLaunchKernelGGL(posfit_band_kernel<float>, dim3((unsigned)((npix + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0,
                     s, src_dev, npix, nb, band, dst_dev);
  DV_HIP(hipGetLastError());
  return OK;
}

int scene_fit_shifts(const double* field_h, int F, const double* stamps_h, int N, int cs, const double* dist_h,
                     double bound, int max_iter, double* shifts_h, double* objective_h, int32_t* iters_h,
                     int32_t* status_h, hipStream_t s) {
  const int64_t one_field[2] = {0, N};
  return scene_fit_shifts_fields(field_h, 1, F, stamps_h, one_field, N, cs, dist_h, bound, max_iter, shifts_h, objective_h,
                                 iters_h, status_h, 0, s);
}

// M fields [M][F][F]; galaxies field_ptr[m] .. field_ptr[m + 1] belong to field m.  A galaxy's fit reads its own field, its
// own stamp and its own workspace only, and every reduction has a fixed order, so its result does not depend on which
// other galaxies or fields share its launch: M fields give what M single-field calls give, bit for bit.
// The fields are uploaded in groups of consecutive fields that fit budget_bytes (0: no limit other than a failed
// allocation); a group's galaxies are fitted, a launch of the plan at a time, before the next group goes up.
int scene_fit_shifts_fields(const double* field_h, int M, int F, const double* stamps_h, const int64_t* field_ptr, int N,
                            int cs, const double* dist_h, double bound, int max_iter, double* shifts_h, double* objective_h,
                            int32_t* iters_h, int32_t* status_h, size_t budget_bytes, hipStream_t s) {
  if (!field_h || !field_ptr || M < 1 || F < 2 || F > 32768 || cs < 1 || cs > F || N < 0 || max_iter < 0 || !(bound >= 0.0) || bound > 1e6 ||
      (N > 0 && (!stamps_h || !dist_h || !shifts_h || !objective_h || !iters_h || !status_h))) {
    set_error("scene_fit_shifts: bad arguments");
    return E_INVALID;
  }
  if (field_ptr[0] != 0 || field_ptr[M] != N) {
    set_error("scene_fit_shifts: field_ptr must run from 0 to the number of galaxies (%d), got %ld .. %ld", N,
              (long)field_ptr[0], (long)field_ptr[M]);
    return E_INVALID;
  }
  for (int m = 0; m < M; ++m)
    if (field_ptr[m + 1] < field_ptr[m]) {
      set_error("scene_fit_shifts: field_ptr decreases at field %d", m);
      return E_INVALID;
    }
  if (N == 0) return OK;
  const size_t STAMP_BUDGET = (size_t)64 << 20;   // stamp doubles per launch (512 MiB)
  PosfitPlan* plan = nullptr;
  DV_TRY(posfit_plan_create(F, cs, N, dist_h, shifts_h, bound, max_iter, &plan));
  PosfitPlanOwner owner(plan);
  std::vector<int32_t> sfield((size_t)N);
  for (int m = 0; m < M; ++m)
    for (int64_t i = field_ptr[m]; i < field_ptr[m + 1]; ++i) sfield[i] = m;

  const size_t img_elems = (size_t)F * F, stamp_elems = (size_t)cs * cs;
  // fields per group
  size_t G = (size_t)M;
  if (budget_bytes) {
    G = std::min<size_t>(G, budget_bytes / (img_elems * sizeof(double)));
    if (G < 1) {
      set_error("scene_fit_shifts: one %d-pixel field (%zu bytes) does not fit the %zu bytes of device memory available "
                "for fields", F, img_elems * sizeof(double), budget_bytes);
      return E_NOMEM;
    }
  }
  // galaxies per launch: at most PF_CHUNK, and at most STAMP_BUDGET doubles of stamps (a few for field-sized stamps)
  const int chunk = (int)std::min<size_t>({(size_t)N, (size_t)PF_CHUNK, std::max<size_t>(1, STAMP_BUDGET / stamp_elems)});
  DevBuf<double> img, tot, stamps, work, out_s, out_j;
  DevBuf<int> out_it, out_st;
  DevBuf<PosfitGeom> dgeo;
  DV_TRY(img.alloc(G * img_elems));
  DV_TRY(tot.alloc(G));
  DV_TRY(stamps.alloc((size_t)chunk * stamp_elems));
  DV_TRY(out_s.alloc((size_t)chunk * 2));
  DV_TRY(out_j.alloc((size_t)chunk));
  DV_TRY(out_it.alloc((size_t)chunk));
  DV_TRY(out_st.alloc((size_t)chunk));
  DV_TRY(dgeo.alloc((size_t)chunk));
  for (int g0 = 0; g0 < M; g0 += (int)G) {
    const int g1 = (int)std::min<size_t>((size_t)M, (size_t)g0 + G);
    const int ga = (int)field_ptr[g0], gb = (int)field_ptr[g1];
    if (ga == gb) continue;                        // no galaxy in these fields
    DV_HIP(hipMemcpyAsync(img, field_h + (size_t)g0 * img_elems, (size_t)(g1 - g0) * img_elems * sizeof(double),
                          hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(posfit_total_sq_kernel, dim3((unsigned)(g1 - g0)), dim3(PF_THREADS), 0, s, img, (long)img_elems, tot);
    DV_HIP(hipGetLastError());
    const int l0 = posfit_plan_layout(plan, ga, gb, chunk, sfield.data(), g0, -1);
    for (int l = l0; l < (int)plan->launches.size(); ++l) {
      const int base = plan->launches[l].base, n = plan->launches[l].n;
      DV_TRY(work.ensure((size_t)plan->launches[l].work));     // (grows to the largest launch so far)
      DV_HIP(hipMemcpyAsync(stamps, stamps_h + (size_t)base * stamp_elems, (size_t)n * stamp_elems * sizeof(double),
                            hipMemcpyHostToDevice, s));
      DV_HIP(hipMemcpyAsync(dgeo, plan->geo.data() + base, (size_t)n * sizeof(PosfitGeom), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(posfit_kernel, dim3((unsigned)n), dim3(PF_THREADS), 0, s, img, F, stamps, cs,
                         dgeo, work, tot, bound, max_iter, out_s, out_j, out_it,
                         out_st);
      DV_HIP(hipGetLastError());
      DV_HIP(hipMemcpyAsync(shifts_h + 2 * (size_t)base, out_s, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
      DV_HIP(hipMemcpyAsync(objective_h + base, out_j, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
      DV_HIP(hipMemcpyAsync(iters_h + base, out_it, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
      DV_HIP(hipMemcpyAsync(status_h + base, out_st, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
      DV_HIP(hipStreamSynchronize(s));             // the device buffers are reused by the next launch
    }
  }
  return OK;
}

}  // namespace dv
