// The deblend kernel of the detector (detect.hip, step 8) and the workgroup helpers it shares with the other detector kernels.
// A header because the kernel is compiled in two translation units: detect.hip holds the instantiation without the object
// columns, detect_objects.hip the one with them, so that the first is compiled exactly as it was
// before the second existed (with both in one unit its register count moved by one).  Include it behind
// `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"

#include <cmath>

namespace dv {

namespace {
constexpr int DT = 256;              // threads of every workgroup here (four waves)
constexpr int DB_LDS = 2048;         // component pixels the deblend keeps in LDS

__device__ __forceinline__ int ald(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int amin(int* p, int v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ast(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void aadd(int* p, int v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum of v over the workgroup in a fixed order; every thread gets the result
template <int K>
__device__ __forceinline__ void blk_sum(double (&v)[K], double* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((s_red[k] + s_red[K + k]) + (s_red[2 * K + k] + s_red[3 * K + k]));
}

// (max v, smallest i at it) over the workgroup; every thread gets the result
__device__ __forceinline__ void blk_argmax(double& v, int& i, double* s_v, int* s_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();
  if (lane == 0) { s_v[wave] = v; s_i[wave] = i; }
  __syncthreads();
  v = s_v[0];
  i = s_i[0];
  for (int w = 1; w < 4; ++w)
    if (s_v[w] > v || (s_v[w] == v && s_i[w] < i)) { v = s_v[w]; i = s_i[w]; }
}

// exclusive prefix sum of x over the workgroup in thread order; total = the sum
__device__ __forceinline__ int blk_scan(int x, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) base += s_w[w];
    total += s_w[w];
  }
  return base + inc - x;
}

__device__ __forceinline__ int blk_isum(int x, int* s_w) {
  int t;
  (void)blk_scan(x, s_w, t);
  return t;
}

// max of every x[k] over the workgroup; every thread gets the results (s_m: 4 * K ints)
template <int K>
__device__ __forceinline__ void blk_imax(int (&x)[K], int* s_m) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x[k] = max(x[k], __shfl_xor(x[k], o, 64));
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_m[wave * K + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] = max(max(s_m[k], s_m[K + k]), max(s_m[2 * K + k], s_m[3 * K + k]));
}

// a pixel counts iff 0 < w < inf (a comparison: NaN does not count), DESIGN 7z
__device__ __forceinline__ bool counts(double w) { return w > 0.0 && w < INFINITY; }

__device__ __forceinline__ int uf_find(int* par, int x) {
  int p = ald(par + x);
  while (p != x) {
    x = p;
    p = ald(par + x);
  }
  return x;
}

// links the larger root under the smaller one; a failed link (the root was linked meanwhile, or the min replaced a parent)
// carries on with the entry it found there, so no connection is lost
__device__ void uf_union(int* par, int a, int b) {
  for (;;) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = amin(par + a, b);
    if (old == a) return;
    a = old;
  }
}

struct DbJob {
  long fbase;          // first pixel of the component's field in the chunk arrays
  long dws, iws;       // double / int scratch offsets
  long slot;           // first catalog slot
  int root, n, c0, c1, r1, cap;
  double T;
};

// object table row (doubles): threshold, mx, my, sxx, sxy, syy, det, A
constexpr int OBJ_D = 8;

// (7zb) what the OBJECTS instantiation of deblend_kernel reads and writes beside the catalogue: wt the plane whose counting
// pixels flag bit 8 asks about (null: the unweighted call), H the field's rows, seg the launch's segmap (null: not asked for),
// oi [slots][OBJ_I] ints: xmin xmax ymin ymax xpeak ypeak xvpeak yvpeak flag and the object's place in the object list,
// od [slots][DET_OBJ_D] doubles: vpeak dflux x_iso y_iso x2 y2 xy
constexpr int OBJ_I = DET_OBJ_I + 1;
struct DbObjects {
  const double* wt;
  int H;
  int* seg;
  int* oi;
  double* od;
};

// OBJECTS = false is the kernel as it was before 7zb, argument for argument.  OBJECTS = true finds its DbObjects behind the
// launch's jobs, in the place of one more job (jobs[gridDim.x]): the host allocates and fills that entry.
static_assert(sizeof(DbObjects) <= sizeof(DbJob) && alignof(DbObjects) <= alignof(DbJob), "DbObjects rides in a job's place");
template <bool OBJECTS>
__global__ __launch_bounds__(DT) void deblend_kernel(const DbJob* __restrict__ jobs, int W, const double* __restrict__ Dall,
                                                     const double* __restrict__ vall, const int* __restrict__ laball,
                                                     int* lidxall, double* dscr, int* iscr, int nthresh, int minarea,
                                                     double cont, int* __restrict__ o_npix, int* __restrict__ o_peakpix,
                                                     double* __restrict__ o_peak, double* __restrict__ o_flux,
                                                     double* __restrict__ o_x, double* __restrict__ o_y,
                                                     int* __restrict__ nobj_out) {
  [[maybe_unused]] DbObjects oo{};
  if constexpr (OBJECTS) oo = *reinterpret_cast<const DbObjects*>(jobs + gridDim.x);
  __shared__ double s_D[DB_LDS];
  __shared__ int s_pix[DB_LDS], s_par[DB_LDS], s_obj[DB_LDS];
  __shared__ double s_red[4 * 8];
  __shared__ int s_w[4], s_i[4], s_b[2];
  [[maybe_unused]] __shared__ int s_m[OBJECTS ? 4 * 5 : 1];
  const int tid = threadIdx.x;
  const DbJob J = jobs[blockIdx.x];
  const int n = J.n, cap = J.cap;
  const bool small = n <= DB_LDS;
  double* dw = dscr + J.dws;
  int* iw = iscr + J.iws;
  // scratch: doubles Dp[n] | nflux[cap] | object table [cap][OBJ_D] | next thresholds [cap]
  //          ints    pix[n] | par[n] | obj[n] | rk[n] | cnt[n] | chid[n] | nodes[cap] | ostate[cap] | nsig[cap]
  double* Dp = small ? s_D : dw;
  double* nflux = dw + n;
  double* otab = nflux + cap;
  double* othr2 = otab + (long)OBJ_D * cap;
  int* pix = small ? s_pix : iw;
  int* par = small ? s_par : iw + n;
  int* obj = small ? s_obj : iw + 2L * n;
  int* rk = iw + 3L * n;
  int* cnt = iw + 4L * n;
  int* chid = iw + 5L * n;
  int* nodes = iw + 6L * n;
  int* ostate = nodes + cap;
  int* nsig = ostate + cap;
  const double* Df = Dall + J.fbase;
  const double* vf = vall + J.fbase;
  const int* labf = laball + J.fbase;
  int* lidx = lidxall + J.fbase;

  // a. the pixels in raster order (scan of the bounding box)
  {
    const int r0 = J.root / W, bw = J.c1 - J.c0 + 1;
    const long total = (long)(J.r1 - r0 + 1) * bw;
    int count = 0;
    for (long base = 0; base < total; base += DT) {
      const long e = base + tid;
      int p = 0;
      bool on = false;
      if (e < total) {
        p = (r0 + (int)(e / bw)) * W + J.c0 + (int)(e % bw);
        on = labf[p] == J.root;
      }
      int tot;
      const int at = count + blk_scan(on ? 1 : 0, s_w, tot);
      if (on) {
        pix[at] = p;
        Dp[at] = Df[p];
        lidx[p] = at;
      }
      count += tot;
    }
  }
  __syncthreads();
  // b. peak and flux of the component
  double P = -INFINITY;
  int pidx = 0x7fffffff;
  double cf[1] = {0.0};
  for (int i = tid; i < n; i += DT) {
    cf[0] += Dp[i];
    if (Dp[i] > P) { P = Dp[i]; pidx = i; }
  }
  blk_argmax(P, pidx, s_red, s_i);
  blk_sum<1>(cf, s_red);
  const double cflux = cf[0];
  for (int i = tid; i < n; i += DT) obj[i] = 0;
  if (tid == 0) otab[0] = J.T;
  int nobj = 1;
  __syncthreads();

  // c. the levels
  for (int k = 1; k < nthresh; ++k) {
    const double t = J.T * pow(P / J.T, (double)k / (double)nthresh);
    int mine = 0;
    for (int i = tid; i < n; i += DT) {
      const bool up = Dp[i] > t;
      ast(par + i, up ? i : -1);                    // words the union-find updates with atomics: atomics only
      ast(cnt + i, 0);
      chid[i] = -1;
      mine += up;
    }
    if (blk_isum(mine, s_w) < minarea) break;      // no node at this level or above (the same for every thread)
    __syncthreads();
    for (int i = tid; i < n; i += DT) {
      if (ald(par + i) < 0) continue;
      const int p = pix[i], r = p / W, c = p - (p / W) * W;
      int q[4];
      int nq = 0;
      if (c > 0) q[nq++] = p - 1;
      if (r > 0) {
        if (c > 0) q[nq++] = p - W - 1;
        q[nq++] = p - W;
        if (c + 1 < W) q[nq++] = p - W + 1;
      }
      for (int a = 0; a < nq; ++a) {
        if (labf[q[a]] != J.root) continue;
        const int j = lidx[q[a]];
        if (ald(par + j) >= 0) uf_union(par, i, j);
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += DT) {
      const int rt = ald(par + i) < 0 ? -1 : uf_find(par, i);
      rk[i] = rt;
      if (rt >= 0) aadd(cnt + rt, 1);
    }
    __syncthreads();
    // the nodes in root order
    int nn = 0;
    for (int base = 0; base < n; base += DT) {
      const int i = base + tid;
      const bool nd = i < n && rk[i] == i && ald(cnt + i) >= minarea;
      int tot;
      const int at = nn + blk_scan(nd ? 1 : 0, s_w, tot);
      if (nd) nodes[at] = i;
      nn += tot;
    }
    __syncthreads();
    // node fluxes in a fixed order; nodes outside every object do not matter
    for (int q = 0; q < nn; ++q) {
      const int rt = nodes[q];
      if (obj[rt] < 0) {
        if (tid == 0) nflux[q] = 0.0;
        continue;
      }
      double a[1] = {0.0};
      for (int i = rt + tid; i < n; i += DT)
        if (rk[i] == rt) a[0] += Dp[i];
      blk_sum<1>(a, s_red);
      if (tid == 0) nflux[q] = a[0];
    }
    __syncthreads();
    // the decision rule (one thread: the object list is short)
    if (tid == 0) {
      for (int o = 0; o < nobj; ++o) nsig[o] = 0;
      for (int q = 0; q < nn; ++q) {
        const int o = obj[nodes[q]];
        if (o >= 0 && nflux[q] > cont * cflux) ++nsig[o];
      }
      int nnew = 0, split = 0;
      for (int o = 0; o < nobj; ++o) {
        if (nsig[o] >= 2) {
          split = 1;
          ostate[o] = -1;
          for (int q = 0; q < nn; ++q) {
            const int rt = nodes[q];
            if (obj[rt] == o && nflux[q] > cont * cflux) {
              chid[rt] = nnew;
              othr2[nnew++] = t;
            }
          }
        } else {
          ostate[o] = nnew;
          othr2[nnew++] = otab[(long)o * OBJ_D];
        }
      }
      for (int o = 0; o < nnew; ++o) otab[(long)o * OBJ_D] = othr2[o];
      s_b[0] = nnew;
      s_b[1] = split;
    }
    __syncthreads();
    const int split = s_b[1];
    nobj = s_b[0];
    if (split) {
      for (int i = tid; i < n; i += DT) {
        const int o = obj[i];
        if (o < 0) continue;
        const int st = ostate[o];
        obj[i] = st >= 0 ? st : (rk[i] >= 0 ? chid[rk[i]] : -1);
      }
    }
    __syncthreads();
  }

  // d. the pixels outside every core go to the object of the largest A exp(-d' S^-1 d / 2)
  if (nobj == 1) {
    for (int i = tid; i < n; i += DT) obj[i] = 0;
  } else {
    for (int o = 0; o < nobj; ++o) {
      double* row = otab + (long)o * OBJ_D;
      const double th = row[0];
      double a[3] = {0.0, 0.0, 0.0};
      double A = -INFINITY;
      int ai = 0x7fffffff;
      for (int i = tid; i < n; i += DT) {
        if (obj[i] != o) continue;
        const double w = Dp[i] - th;
        const int p = pix[i];
        a[0] += w;
        a[1] += w * (p - (p / W) * W);
        a[2] += w * (p / W);
        if (Dp[i] > A) { A = Dp[i]; ai = i; }
      }
      blk_sum<3>(a, s_red);
      blk_argmax(A, ai, s_red + 12, s_i);
      const double mx = a[1] / a[0], my = a[2] / a[0];
      double b[3] = {0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += DT) {
        if (obj[i] != o) continue;
        const double w = Dp[i] - th;
        const int p = pix[i];
        const double dx = (p - (p / W) * W) - mx, dy = (p / W) - my;
        b[0] += w * dx * dx;
        b[1] += w * dx * dy;
        b[2] += w * dy * dy;
      }
      blk_sum<3>(b, s_red);
      if (tid == 0) {
        const double sxx = b[0] / a[0] + 1.0 / 12.0, sxy = b[1] / a[0], syy = b[2] / a[0] + 1.0 / 12.0;
        row[1] = mx;
        row[2] = my;
        row[3] = sxx;
        row[4] = sxy;
        row[5] = syy;
        row[6] = sxx * syy - sxy * sxy;
        row[7] = A;
      }
      __syncthreads();
    }
    for (int i = tid; i < n; i += DT) {
      if (obj[i] >= 0) continue;
      const int p = pix[i];
      const double cx = p - (p / W) * W, cy = p / W;
      double best = -INFINITY;
      int bo = 0;
      for (int o = 0; o < nobj; ++o) {
        const double* row = otab + (long)o * OBJ_D;
        const double ex = cx - row[1], ey = cy - row[2];
        const double q = (row[5] * ex * ex - 2.0 * row[4] * ex * ey + row[3] * ey * ey) / row[6];
        const double sc = row[7] * exp(-0.5 * q);
        if (sc > best) { best = sc; bo = o; }
      }
      rk[i] = bo;
    }
    __syncthreads();
    for (int i = tid; i < n; i += DT)
      if (obj[i] < 0) obj[i] = rk[i];
  }
  __syncthreads();

  // e. the catalog, then the objects ordered by peak pixel
  for (int o = 0; o < nobj; ++o) {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // npix, sum v, sum v c, sum v r, sum c, sum r
    double pk = -INFINITY;
    int pi = 0x7fffffff;
    for (int i = tid; i < n; i += DT) {
      if (obj[i] != o) continue;
      const int p = pix[i];
      const double v = vf[p], c = p - (p / W) * W, r = p / W;
      a[0] += 1.0;
      a[1] += v;
      a[2] += v * c;
      a[3] += v * r;
      a[4] += c;
      a[5] += r;
      if (Dp[i] > pk) { pk = Dp[i]; pi = i; }
    }
    blk_sum<6>(a, s_red);
    blk_argmax(pk, pi, s_red + 24, s_i);
    if (tid == 0) {
      const long sl = J.slot + o;
      o_npix[sl] = (int)a[0];
      o_peakpix[sl] = pix[pi];
      o_peak[sl] = pk;
      o_flux[sl] = a[1];
      o_x[sl] = a[1] > 0.0 ? a[2] / a[1] : a[4] / a[0];
      o_y[sl] = a[1] > 0.0 ? a[3] / a[1] : a[5] / a[0];
    }
    __syncthreads();
    if constexpr (OBJECTS) {                          // (7zb) the box, the peak of v, the isophotal moments, the flags
      double d[3] = {0.0, 0.0, 0.0};                  // sum D, sum D c, sum D r
      double vk = -INFINITY;
      int vi = 0x7fffffff;
      int bx[5] = {-0x7fffffff, -0x7fffffff, -0x7fffffff, -0x7fffffff, 0};   // -xmin, xmax, -ymin, ymax, bit 8
      const double* wf = oo.wt ? oo.wt + J.fbase : nullptr;
      for (int i = tid; i < n; i += DT) {
        if (obj[i] != o) continue;
        const int p = pix[i], r = p / W, c = p - (p / W) * W;
        const double Dv = Dp[i], v = vf[p];
        d[0] += Dv;
        d[1] += Dv * c;
        d[2] += Dv * r;
        if (v > vk) { vk = v; vi = i; }
        bx[0] = max(bx[0], -c);
        bx[1] = max(bx[1], c);
        bx[2] = max(bx[2], -r);
        bx[3] = max(bx[3], r);
        if (wf) {
          for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
              const int rr = r + dr, cc = c + dc;
              if ((dr != 0 || dc != 0) && rr >= 0 && rr < oo.H && cc >= 0 && cc < W && !counts(wf[(long)rr * W + cc])) bx[4] = 1;
            }
        }
      }
      blk_sum<3>(d, s_red);
      blk_argmax(vk, vi, s_red + 12, s_i);
      blk_imax<5>(bx, s_m);
      const double xi = d[1] / d[0], yi = d[2] / d[0];
      double m2[3] = {0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += DT) {
        if (obj[i] != o) continue;
        const int p = pix[i];
        const double dx = (p - (p / W) * W) - xi, dy = (p / W) - yi, Dv = Dp[i];
        m2[0] += (Dv * dx) * dx;
        m2[1] += (Dv * dy) * dy;
        m2[2] += (Dv * dx) * dy;
      }
      blk_sum<3>(m2, s_red);
      if (tid == 0) {
        const long sl = J.slot + o;
        int* ri = oo.oi + sl * OBJ_I;
        double* rd = oo.od + sl * DET_OBJ_D;
        double x2 = m2[0] / d[0], y2 = m2[1] / d[0];
        const double xy = m2[2] / d[0];
        const int xmin = -bx[0], xmax = bx[1], ymin = -bx[2], ymax = bx[3];
        int flag = nobj > 1 ? 1 : 0;
        if (xmin == 0 || ymin == 0 || xmax == W - 1 || ymax == oo.H - 1) flag |= 2;
        if (x2 * y2 - xy * xy < 1.0 / 144.0) {
          x2 += 1.0 / 12.0;
          y2 += 1.0 / 12.0;
          flag |= 4;
        }
        if (bx[4]) flag |= 8;
        const int pp = pix[pi], vp = pix[vi];
        ri[0] = xmin; ri[1] = xmax; ri[2] = ymin; ri[3] = ymax;
        ri[4] = pp - (pp / W) * W; ri[5] = pp / W;
        ri[6] = vp - (vp / W) * W; ri[7] = vp / W;
        ri[8] = flag; ri[9] = o;
        rd[0] = vk; rd[1] = d[0]; rd[2] = xi; rd[3] = yi; rd[4] = x2; rd[5] = y2; rd[6] = xy;
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const long b = J.slot;
    for (int o = 1; o < nobj; ++o) {                 // insertion sort of the slots by peak pixel
      const int kp = o_peakpix[b + o], kn = o_npix[b + o];
      const double k1 = o_peak[b + o], k2 = o_flux[b + o], k3 = o_x[b + o], k4 = o_y[b + o];
      [[maybe_unused]] int ki[OBJ_I];
      [[maybe_unused]] double kd[DET_OBJ_D];
      if constexpr (OBJECTS) {
        for (int e = 0; e < OBJ_I; ++e) ki[e] = oo.oi[(b + o) * OBJ_I + e];
        for (int e = 0; e < DET_OBJ_D; ++e) kd[e] = oo.od[(b + o) * DET_OBJ_D + e];
      }
      int q = o;
      while (q > 0 && o_peakpix[b + q - 1] > kp) {
        if constexpr (OBJECTS) {
          for (int e = 0; e < OBJ_I; ++e) oo.oi[(b + q) * OBJ_I + e] = oo.oi[(b + q - 1) * OBJ_I + e];
          for (int e = 0; e < DET_OBJ_D; ++e) oo.od[(b + q) * DET_OBJ_D + e] = oo.od[(b + q - 1) * DET_OBJ_D + e];
        }
        o_peakpix[b + q] = o_peakpix[b + q - 1];
        o_npix[b + q] = o_npix[b + q - 1];
        o_peak[b + q] = o_peak[b + q - 1];
        o_flux[b + q] = o_flux[b + q - 1];
        o_x[b + q] = o_x[b + q - 1];
        o_y[b + q] = o_y[b + q - 1];
        --q;
      }
      o_peakpix[b + q] = kp;
      o_npix[b + q] = kn;
      o_peak[b + q] = k1;
      o_flux[b + q] = k2;
      o_x[b + q] = k3;
      o_y[b + q] = k4;
      if constexpr (OBJECTS) {
        for (int e = 0; e < OBJ_I; ++e) oo.oi[(b + q) * OBJ_I + e] = ki[e];
        for (int e = 0; e < DET_OBJ_D; ++e) oo.od[(b + q) * DET_OBJ_D + e] = kd[e];
      }
    }
    nobj_out[blockIdx.x] = nobj;
    if constexpr (OBJECTS)                            // the catalogue rank of every entry of the object list
      for (int o = 0; o < nobj; ++o) nsig[oo.oi[(b + o) * OBJ_I + DET_OBJ_I]] = o;
  }
  if constexpr (OBJECTS) {
    // the segmap numbers within the component; lidx names the job, whose base seg_base_kernel adds in the next launch
    if (oo.seg) {
      __syncthreads();
      int* seg = oo.seg + J.fbase;
      for (int i = tid; i < n; i += DT) {
        const int p = pix[i];
        seg[p] = nsig[obj[i]] + 1;
        lidx[p] = (int)blockIdx.x;
      }
    }
  }
}

}  // namespace

// deblend_kernel<true> on nj jobs (detect_objects.hip); djobs holds nj + 1 entries, the last one the DbObjects
int deblend_objects_launch(long nj, hipStream_t s, const void* djobs, int W, const double* D, const double* v, const int* lab,
                           int* lidx, double* dscr, int* iscr, int nthresh, int minarea, double cont, int* o_npix, int* o_pp,
                           double* o_peak, double* o_flux, double* o_x, double* o_y, int* nobj);

}  // namespace dv
