// Row sets, the field-table preamble and the chunk walkers of the catalogue calls (rows.h).  Host code only.
#include "rows.h"

#include <algorithm>
#include <cstring>
#include <new>

#ifdef DV_DEBUG_EXPORTS
#include "../../include/debvader_hip_debug.h"
#endif

namespace dv {

#ifdef DV_DEBUG_EXPORTS
namespace {
int64_t g_cap_rows = 0, g_cap_fields = 0;               // dv_debug_scene_limits (0: no cap)
}  // namespace
#endif

size_t Rows::bytes() const {
  size_t b = 0;
  for (int i = 0; i < ncols; ++i) b += cols[i].width;
  return b;
}

int Rows::alloc(int64_t n) {
  for (int i = 0; i < ncols; ++i) {
    DV_TRY(mem[i].alloc((size_t)n * cols[i].width));
    *cols[i].dev = mem[i].get();
  }
  return OK;
}

void Rows::advance(int64_t r) {
  for (int i = 0; i < ncols; ++i)
    if (*cols[i].dev) *cols[i].dev = (char*)*cols[i].dev + (size_t)r * cols[i].width;
}

int Rows::upload(int64_t r, int64_t n, hipStream_t s) const {
  for (int i = 0; i < ncols; ++i) {
    const Column& c = cols[i];
    if (c.host && n > 0) DV_HIP(hipMemcpyAsync(*c.dev, c.host + (size_t)r * c.width, (size_t)n * c.width, hipMemcpyHostToDevice, s));
  }
  return OK;
}

int Rows::download(int64_t r, int64_t n, hipStream_t s) const {
  for (int i = 0; i < ncols; ++i) {
    const Column& c = cols[i];
    if (c.host && n > 0) DV_HIP(hipMemcpyAsync(c.host + (size_t)r * c.width, *c.dev, (size_t)n * c.width, hipMemcpyDeviceToHost, s));
  }
  return OK;
}

void* RowStage::add(void* dest, size_t width, int64_t n) {
  Col& c = cols[ncols++];
  c.dest = (char*)dest;
  c.width = width;
  c.rows.assign((size_t)n * width, 0);
  return c.rows.data();
}

void RowStage::take(Rows& r, int64_t n) {
  for (int i = 0; i < r.ncols; ++i)
    if (r.cols[i].host) r.cols[i].host = (char*)add(r.cols[i].host, r.cols[i].width, n);
}

void RowStage::scatter(const int* rowmap, int64_t n) const {
  for (int i = 0; i < ncols; ++i)
    for (int64_t k = 0; k < n; ++k)
      std::memcpy(cols[i].dest + (size_t)rowmap[k] * cols[i].width, cols[i].rows.data() + (size_t)k * cols[i].width, cols[i].width);
}

int place_check(const char* who, int64_t i, const int32_t* places) {
  const int pr = places[2 * i], pc = places[2 * i + 1];
  if (pr < -(1 << 28) || pr > (1 << 28) || pc < -(1 << 28) || pc > (1 << 28)) {
    set_error("%s: placement %ld (%d,%d) out of range", who, (long)i, pr, pc);
    return E_INVALID;
  }
  return OK;
}

int field_tables(const char* who, const char* noun, int M, const int64_t* field_ptr, int64_t N, const int* F,
                 const int32_t* places, std::vector<int32_t>* sfield, std::vector<int>* fptr32) {
  if (N >= ((int64_t)1 << 31)) {
    set_error("%s: %ld %s, at most 2^31 - 1 per call", who, (long)N, noun);
    return E_INVALID;
  }
  if (F && (*F < 1 || *F > 32768)) {
    set_error("%s: fields of %d pixels, 1 .. 32768 are taken", who, *F);
    return E_INVALID;
  }
  if (field_ptr[0] != 0 || field_ptr[M] != N) {
    set_error("%s: field_ptr must run from 0 to the number of %s (%ld), got %ld .. %ld", who, noun, (long)N,
              (long)field_ptr[0], (long)field_ptr[M]);
    return E_INVALID;
  }
  for (int f = 0; f < M; ++f)                          // the whole table before anything is indexed by it
    if (field_ptr[f + 1] < field_ptr[f]) {
      set_error("%s: field_ptr decreases at field %d (%ld after %ld)", who, f, (long)field_ptr[f + 1], (long)field_ptr[f]);
      return E_INVALID;
    }
  if (places)
    for (int64_t i = 0; i < N; ++i) DV_TRY(place_check(who, i, places));
  try {
    if (sfield) sfield->assign((size_t)N, 0);
    if (fptr32) fptr32->assign((size_t)M + 1, 0);
  } catch (const std::bad_alloc&) {
    set_error("%s: no host memory for the field table of %ld %s", who, (long)N, noun);
    return E_NOMEM;
  }
  for (int f = 0; f <= M && fptr32; ++f) (*fptr32)[(size_t)f] = (int)field_ptr[f];
  for (int f = 0; f < M && sfield; ++f)
    for (int64_t i = field_ptr[f]; i < field_ptr[f + 1]; ++i) (*sfield)[(size_t)i] = f;
  return OK;
}

int scene_limits(int share, size_t fixed, size_t row_bytes, size_t field_bytes, int64_t* chunk, int64_t* gmax) {
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t part = free_b / (size_t)share;
  *chunk = (int64_t)std::max<size_t>(1, (part > fixed ? part - fixed : 0) / std::max<size_t>(row_bytes, 1));
  *gmax = field_bytes ? (int64_t)std::max<size_t>(1, part / field_bytes) : 0;
#ifdef DV_DEBUG_EXPORTS
  if (g_cap_rows > 0) *chunk = std::min(*chunk, g_cap_rows);
  if (g_cap_fields > 0 && field_bytes) *gmax = std::min(*gmax, g_cap_fields);
#endif
  return OK;
}

int walk_rows(int64_t N, int64_t max_rows, size_t fixed, Rows& in, Rows& out, hipStream_t s,
              const std::function<int(int64_t base, int n)>& body) {
  if (N <= 0) return OK;
  StreamDrain drain(s);                                // (the rows are the caller's: they outlive this scope)
  int64_t chunk = 0, gmax = 0;
  DV_TRY(scene_limits(2, fixed, in.bytes() + out.bytes(), 0, &chunk, &gmax));
  chunk = std::max<int64_t>(1, std::min<int64_t>({chunk, N, max_rows}));
  DV_TRY(in.alloc(chunk));
  DV_TRY(out.alloc(chunk));
  for (int64_t base = 0; base < N; base += chunk) {
    const int n = (int)std::min<int64_t>(chunk, N - base);
    DV_TRY(in.upload(base, n, s));
    DV_TRY(body(base, n));
    DV_TRY(out.download(base, n, s));
    DV_HIP(hipStreamSynchronize(s));                   // the device buffers are reused by the next chunk
  }
  drain.dismiss();
  return OK;
}

int walk_field_rows(int64_t N, const int32_t* sfield, FieldStacks& f, Rows& in, Rows& out, hipStream_t s,
                    const std::function<int(int64_t base, int n, int fa)>& body) {
  if (N <= 0) return OK;
  DevBuf<double> model, data;
  StreamDrain drain(s);
  const size_t fb = f.felems * sizeof(double);
  int64_t chunk = 0, gmax = 0;
  DV_TRY(scene_limits(4, 0, in.bytes() + out.bytes(), fb * (f.data_h ? 2 : 1), &chunk, &gmax));
  chunk = std::max<int64_t>(1, std::min<int64_t>({chunk, N, (int64_t)1 << 20}));
  gmax = std::max<int64_t>(1, std::min<int64_t>(gmax, f.M));
  DV_TRY(in.alloc(chunk));
  DV_TRY(out.alloc(chunk));
  DV_TRY(model.alloc((size_t)gmax * f.felems));
  if (f.data_h) DV_TRY(data.alloc((size_t)gmax * f.felems));
  f.model_d = model;
  f.data_d = f.data_h ? data.get() : nullptr;
  for (int64_t base = 0; base < N;) {
    const int fa = sfield[(size_t)base];
    int n = 0;                                         // rows of at most gmax fields from fa on (at least one)
    while (n < chunk && base + n < N && (int64_t)sfield[(size_t)(base + n)] - fa < gmax) ++n;
    const size_t nf = (size_t)(sfield[(size_t)(base + n - 1)] - fa + 1);
    DV_HIP(hipMemcpyAsync(model, f.model_h + (size_t)fa * f.felems, nf * fb, hipMemcpyHostToDevice, s));
    if (f.data_h) DV_HIP(hipMemcpyAsync(data, f.data_h + (size_t)fa * f.felems, nf * fb, hipMemcpyHostToDevice, s));
    DV_TRY(in.upload(base, n, s));
    DV_TRY(body(base, n, fa));
    DV_TRY(out.download(base, n, s));
    DV_HIP(hipStreamSynchronize(s));                   // the device buffers are reused by the next chunk
    base += n;
  }
  drain.dismiss();
  f.model_d = f.data_d = nullptr;
  return OK;
}

int plan_field_runs(const int64_t* field_ptr, int M, size_t row_bytes, size_t field_bytes, size_t budget, int64_t max_stamps,
                    int64_t max_fields, FieldRuns* runs, size_t* need) {
  std::vector<int> cuts{0};
  size_t cmax_s = 0, cmax_f = 0;
  for (int f = 0; f < M;) {
    size_t bytes = 0;
    int g = f;
    while (g < M) {
      const size_t add = (size_t)(field_ptr[g + 1] - field_ptr[g]) * row_bytes + field_bytes;
      if (g > f && (bytes + add > budget || (max_fields > 0 && g - f >= max_fields) ||
                    (max_stamps > 0 && field_ptr[g + 1] - field_ptr[f] > max_stamps)))
        break;
      bytes += add;
      ++g;
    }
    if (bytes > budget) {
      *need = bytes;
      return f;
    }
    cmax_s = std::max(cmax_s, (size_t)(field_ptr[g] - field_ptr[f]));
    cmax_f = std::max(cmax_f, (size_t)(g - f));
    cuts.push_back(g);
    f = g;
  }
  runs->first = std::move(cuts);
  runs->max_rows = cmax_s;
  runs->max_fields = cmax_f;
  return -1;
}

JointOrder joint_order(const std::vector<std::vector<int>>& pass_fptr, int M) {
  JointOrder o;
  for (int f = 0; f < M; ++f) {
    o.fptr64.push_back((int64_t)o.rowmap.size());
    size_t base = 0;                                   // the resident row of the pass's row 0
    for (const std::vector<int>& p : pass_fptr) {
      for (int i = p[(size_t)f]; i < p[(size_t)f + 1]; ++i) {
        o.rowmap.push_back((int)(base + (size_t)i));
        o.sfield.push_back(f);
      }
      base += (size_t)p[(size_t)M];
    }
  }
  o.fptr64.push_back((int64_t)o.rowmap.size());
  o.fptr32.assign(o.fptr64.begin(), o.fptr64.end());
  return o;
}

std::vector<int32_t> JointOrder::places(const int32_t* resident) const {
  std::vector<int32_t> p(rowmap.size() * 2);
  for (size_t k = 0; k < rowmap.size(); ++k) {
    p[2 * k] = resident[2 * (size_t)rowmap[k]];
    p[2 * k + 1] = resident[2 * (size_t)rowmap[k] + 1];
  }
  return p;
}

int walk_whole_fields(const char* who, int M, const int64_t* field_ptr, int64_t N, WholeFields& f, FieldStamps& v, Rows& in,
                      Rows& out, hipStream_t s,
                      const std::function<int(const FieldStamps& v, int fa, int nf, int64_t r0, const int* fptr_h)>& body) {
  if (N == 0 && !f.empty_runs) return OK;
  const double* const stack_h[3] = {f.model_h, f.data_h, f.weight_h};
  const double** const stack_v[3] = {&v.model, &v.data, &v.weight};
  const size_t felems = (size_t)v.F * v.F * v.nb, fb = felems * sizeof(double);
  size_t per_field = sizeof(int) + f.field_bytes;     // (the run's field_ptr)
  for (const double* h : stack_h)
    if (h) per_field += fb;
  const size_t per_row = in.bytes() + out.bytes() + sizeof(int) + f.row_bytes;   // (the field of the row)
  size_t free_b = 0, total_b = 0;
  DV_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 2 > f.fixed ? free_b / 2 - f.fixed : 0;
  int64_t cap_rows = 0, cap_fields = 0;
#ifdef DV_DEBUG_EXPORTS
  cap_rows = g_cap_rows;
  cap_fields = g_cap_fields;
#endif
  FieldRuns runs;
  size_t need = 0;
  const int refused = plan_field_runs(field_ptr, M, per_row, per_field, budget, cap_rows, cap_fields, &runs, &need);
  if (refused >= 0) {
    set_error("%s: field %d with its %ld stamps needs %zu bytes of device memory, %zu are available", who, refused,
              (long)(field_ptr[refused + 1] - field_ptr[refused]), need, budget);
    return E_NOMEM;
  }
  f.max_rows = runs.max_rows;
  f.max_fields = runs.max_fields;
  DevBuf<int> sf, fptr;
  DevBuf<double> stack[3];
  DV_TRY(in.alloc((int64_t)runs.max_rows));
  DV_TRY(out.alloc((int64_t)runs.max_rows));
  DV_TRY(sf.alloc(runs.max_rows));
  DV_TRY(fptr.alloc(runs.max_fields + 1));
  for (int k = 0; k < 3; ++k) {
    if (stack_h[k]) DV_TRY(stack[k].alloc(runs.max_fields * felems));
    *stack_v[k] = stack_h[k] ? stack[k].get() : nullptr;
  }
  v.sfield = sf;
  v.fptr = fptr;
  v.f0 = 0;
  std::vector<int> sf_h, fptr_h;
  StreamDrain drain(s);
  for (size_t k = 0; k + 1 < runs.first.size(); ++k) {
    const int fa = runs.first[k], fz = runs.first[k + 1];   // fields fa .. fz - 1, their rows counted from the run's first
    const int64_t r0 = field_ptr[fa], n = field_ptr[fz] - r0;
    if (n == 0 && !f.empty_runs) continue;
    fptr_h.assign((size_t)(fz - fa) + 1, 0);
    sf_h.assign((size_t)n, 0);
    for (int g = fa; g < fz; ++g) {
      fptr_h[(size_t)(g - fa) + 1] = (int)(field_ptr[g + 1] - r0);
      for (int64_t i = field_ptr[g]; i < field_ptr[g + 1]; ++i) sf_h[(size_t)(i - r0)] = g - fa;
    }
    DV_TRY(in.upload(r0, n, s));
    if (n > 0) DV_HIP(hipMemcpyAsync(sf, sf_h.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    DV_HIP(hipMemcpyAsync(fptr, fptr_h.data(), fptr_h.size() * sizeof(int), hipMemcpyHostToDevice, s));
    for (int j = 0; j < 3; ++j)
      if (stack_h[j])
        DV_HIP(hipMemcpyAsync(stack[j], stack_h[j] + (size_t)fa * felems, (size_t)(fz - fa) * fb, hipMemcpyHostToDevice, s));
    DV_TRY(body(v, fa, fz - fa, r0, fptr_h.data()));
    DV_TRY(out.download(r0, n, s));
    DV_HIP(hipStreamSynchronize(s));                   // the device buffers and the host tables are reused by the next run
  }
  drain.dismiss();
  return OK;
}

}  // namespace dv

#ifdef DV_DEBUG_EXPORTS
int dv_debug_scene_limits(int64_t max_stamps, int64_t max_fields) {
  dv::g_cap_rows = max_stamps;
  dv::g_cap_fields = max_fields;
  return DV_OK;
}
#endif
