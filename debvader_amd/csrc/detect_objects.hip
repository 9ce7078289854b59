// The deblend kernel with the object columns and the segmap: deblend_kernel<true> of deblend_dev.h in
// a translation unit of its own, see there.
#include "common.h"

#pragma clang fp contract(off)

#include "deblend_dev.h"

namespace dv {

int deblend_objects_launch(long nj, hipStream_t s, const void* djobs, int W, const double* D, const double* v, const int* lab,
                           int* lidx, double* dscr, int* iscr, int nthresh, int minarea, double cont, int* o_npix, int* o_pp,
                           double* o_peak, double* o_flux, double* o_x, double* o_y, int* nobj) {
  hipLaunchKernelGGL(deblend_kernel<true>, dim3((unsigned)nj), dim3(DT), 0, s, (const DbJob*)djobs, W, D, v, lab, lidx, dscr, iscr,
                     nthresh, minarea, cont, o_npix, o_pp, o_peak, o_flux, o_x, o_y, nobj);
  DV_HIP(hipGetLastError());
  return OK;
}

}  // namespace dv
